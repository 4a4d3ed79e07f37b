// lpd_clean.hip -- road removal and range crop for raw scans: what stands between a LiDAR driver's buffer and lpd_make_submaps.  The
// reference's submaps come "with the road removed" from an offline preprocessing step that is not part of it; this file is that
// step for a ragged batch, on the device, without a read-back.  Definition: include/lpd_hip.h; arithmetic: lpd_clean_math.h.
//
// lpd_road_planes, a chain of small launches on one stream (CL_T = 256 threads; a "chunk" is LPD_CLEAN_CHUNK = 1024 rows of one scan,
// LPD_CLEAN_LANE_ROWS = 4 rows per lane, row c0 + k * 256 + tid in slot k: coalesced, and ascending in (k, wave, lane)):
//   hypotheses  one workgroup per scan: thread h draws its three rows with Philox, tests them and writes the plane (a, b, c, valid)
//               into the table hyp[b][h]; zeroes the scan's scores and sums; starts info
//   score       grid (chunk, scan).  A lane keeps its four rows in registers (a row that is not live becomes (0, 0, NaN): its residual
//               is NaN and fails the comparison, no mask in the loop).  The loop is over h, four at a time: the planes are read with
//               wave-uniform addresses (scalar loads, a plane is three SGPRs), four loads in flight in front of the arithmetic.  Per h
//               and row slot: 2 mul + 3 add/sub + 1 compare with |.|, __ballot + popcount -> a wave-uniform count; ONE LDS integer add
//               per wave and h; at the end one global integer atomic per workgroup and h with a nonzero count.  Invalid hypotheses
//               are skipped (a uniform branch).  The live rows are counted the same way into info[b][0].
//   select      one workgroup per scan: max over the valid h of (S << 10 | 1023 - h) -- the largest S, ties to the lowest h; the
//               status; plane and info; the origin p0 of h* (its rows are drawn again)
//   moments     (refine) grid (chunk, scan): the nine sums of the inliers of h* in 64-bit integers: per lane, xor tree over the wave,
//               waves in LDS, one 64-bit integer atomic per workgroup and sum.  Integer sums: exact, so independent of the order.
//   solve       (refine) one thread per scan: lpd_clean_solve in float64
//   recount     (refine) grid (chunk, scan): inliers of the refined plane -> info[b][3]
// lpd_clean_count / lpd_clean_fill are ONE templated kernel over (chunk, scan), as radius_kernel<FILL> of lpd_places.hip: the same
// predicate in both; the place of a kept row = block base (the caller's exclusive scan of the counts) + the counts of the (slot, wave)
// pairs in front (16 numbers in LDS) + the popcount of the ballot's lanes below.  Stable by construction, no sort.
// No float atomics anywhere; integer atomics only: the same bits in every launch.
//
// Registers / LDS: score holds 12 floats of rows and 16 SGPRs of planes, 4 KiB + 4 B of counters; moments 18 VGPRs of sums and 288 B;
// nothing here limits the occupancy (8 waves per SIMD), which is what hides the scalar-load latency of the table.
#include <math.h>

#include "lpd_common.h"
#include "lpd_clean_math.h"

namespace {

constexpr int CL_T = 256;
constexpr int CL_WAVES = CL_T / 64;
constexpr int CL_R = LPD_CLEAN_LANE_ROWS;
constexpr int CL_CH = LPD_CLEAN_CHUNK;
static_assert(CL_T * CL_R == CL_CH, "rows of a workgroup");
static_assert(LPD_CLEAN_MAX_H == 1024, "the choice key keeps h in 10 bits");

struct ClK {      // LpdCleanParams as the kernels want it
    float rmin2, rmax2, z_lo, z_hi, band_lo, band_hi, tau, min_det, slope2, clearance;
    int H, min_inliers;
    uint32_t seed_lo, seed_hi;
};

struct ClSel { float a, b, c, ox, oy, oz; int status, pad; };      // status: 0 no road, 1 the plane of h*, 2 refined

// workspace: hyp [B][H] float4, scores [B][H] int32, sums [B][16] int64, sel [B]
struct ClWs {
    float4* hyp;
    int32_t* scores;
    unsigned long long* sums;
    ClSel* sel;
};

inline size_t cl_up(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t cl_ws_bytes(int B, int H)
{
    return cl_up((size_t)B * H * 16) + cl_up((size_t)B * H * 4) + cl_up((size_t)B * 16 * 8) + cl_up((size_t)B * sizeof(ClSel));
}
inline ClWs cl_ws(void* ws, int B, int H)
{
    unsigned char* p = (unsigned char*)ws;
    ClWs w;
    w.hyp = (float4*)p;
    p += cl_up((size_t)B * H * 16);
    w.scores = (int32_t*)p;
    p += cl_up((size_t)B * H * 4);
    w.sums = (unsigned long long*)p;
    p += cl_up((size_t)B * 16 * 8);
    w.sel = (ClSel*)p;
    return w;
}

// rows of scan b, or false: offsets the definition excludes (negative, empty, longer than max_len <= 2^20, or ending behind the
// table) -- such a scan is never read
__device__ __forceinline__ bool cl_scan(const int32_t* __restrict__ offsets, int b, int rows, int max_len, long long* o0, int* n)
{
    const long long a = offsets[b], e = offsets[b + 1];
    *o0 = a;
    *n = (int)(e - a);
    return a >= 0 && e - a >= 1 && e - a <= max_len && e <= rows;
}

// the lane's rows of a chunk; a row that is not live (or lies behind the scan's end) becomes (0, 0, NaN) and `live` says so
struct ClRows { float x[CL_R], y[CL_R], z[CL_R]; bool live[CL_R]; };

__device__ __forceinline__ ClRows cl_load(const float* __restrict__ p, int ld, int n, int c0, int tid, const ClK& K)
{
    ClRows r;
#pragma unroll
    for (int k = 0; k < CL_R; ++k) {
        const int i = c0 + k * CL_T + tid;
        float x = 0.0f, y = 0.0f, z = NAN;
        bool live = false;
        if (i < n) {
            const float* q = p + (size_t)i * ld;
            x = q[0]; y = q[1]; z = q[2];
            live = lpd_clean_live(x, y, z, K.rmin2, K.rmax2, K.z_lo, K.z_hi);
        }
        r.live[k] = live;
        r.x[k] = live ? x : 0.0f;
        r.y[k] = live ? y : 0.0f;
        r.z[k] = live ? z : NAN;
    }
    return r;
}

__global__ __launch_bounds__(CL_T) void hyp_kernel(const float* __restrict__ points, int ld, int rows, const int32_t* __restrict__ offsets,
                                                   int max_len, ClK K, ClWs W, float* __restrict__ plane, int32_t* __restrict__ info)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    long long o0;
    int n;
    const bool ok = cl_scan(offsets, b, rows, max_len, &o0, &n);
    if (tid < 4) {
        plane[4 * b + tid] = 0.0f;
        info[4 * b + tid] = ok ? (tid == 1 ? -1 : 0) : (tid < 2 ? -1 : 0);      // (n_live = 0 so far, -1, 0, 0) / (-1, -1, 0, 0)
    }
    if (tid < 16) W.sums[16 * b + tid] = 0ull;
    if (tid == 0) W.sel[b] = ClSel{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0, 0};
    if (!ok) return;
    const float* p = points + (size_t)o0 * ld;
    for (int h = tid; h < K.H; h += CL_T) {
        const LpdCleanRows d = lpd_clean_draw((uint32_t)h, (uint32_t)b, (uint32_t)n, K.seed_lo, K.seed_hi);
        float q[3][3];
        bool good = true;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float* s = p + (size_t)d.i[j] * ld;      // d.i[j] < n
            q[j][0] = s[0]; q[j][1] = s[1]; q[j][2] = s[2];
            good = good && lpd_clean_live(q[j][0], q[j][1], q[j][2], K.rmin2, K.rmax2, K.z_lo, K.z_hi) &&
                   lpd_clean_in_band(q[j][2], K.band_lo, K.band_hi);
        }
        const LpdCleanPlane P = lpd_clean_triple(q[0], q[1], q[2], good, K.min_det, K.slope2);
        W.hyp[(size_t)b * K.H + h] = make_float4(P.a, P.b, P.c, P.valid ? 1.0f : 0.0f);
        W.scores[(size_t)b * K.H + h] = 0;
    }
}

__global__ __launch_bounds__(CL_T) void score_kernel(const float* __restrict__ points, int ld, int rows, const int32_t* __restrict__ offsets,
                                                     int max_len, ClK K, const float4* __restrict__ hyp, int32_t* __restrict__ scores,
                                                     int32_t* __restrict__ info)
{
    __shared__ int cnt[LPD_CLEAN_MAX_H + 1];      // [h], and the live rows in [H]
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, H = K.H;
    const int c0 = blockIdx.x * CL_CH;
    long long o0;
    int n;
    if (!cl_scan(offsets, b, rows, max_len, &o0, &n) || c0 >= n) return;      // uniform over the workgroup
    for (int h = tid; h <= H; h += CL_T) cnt[h] = 0;
    const ClRows r = cl_load(points + (size_t)o0 * ld, ld, n, c0, tid, K);
    int nl = 0;
#pragma unroll
    for (int k = 0; k < CL_R; ++k) nl += __popcll(__ballot(r.live[k]));
    __syncthreads();
    if (lane == 0 && nl) atomicAdd(&cnt[H], nl);
    if (nl) {      // a wave without a live row adds nothing to any score
        const float4* hb = hyp + (size_t)b * H;
        for (int h0 = 0; h0 < H; h0 += 4) {
            float4 P[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) P[j] = hb[h0 + j < H ? h0 + j : H - 1];      // uniform addresses: four loads under way
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (h0 + j < H && P[j].w != 0.0f) {
                    int c = 0;
#pragma unroll
                    for (int k = 0; k < CL_R; ++k)
                        c += __popcll(__ballot(lpd_clean_inlier(lpd_clean_residual(r.x[k], r.y[k], r.z[k], P[j].x, P[j].y, P[j].z), K.tau)));
                    if (lane == 0 && c) atomicAdd(&cnt[h0 + j], c);
                }
            }
        }
    }
    __syncthreads();
    for (int h = tid; h <= H; h += CL_T) {
        const int v = cnt[h];
        if (v) atomicAdd(h < H ? &scores[(size_t)b * H + h] : &info[4 * b], v);
    }
}

__global__ __launch_bounds__(CL_T) void select_kernel(const float* __restrict__ points, int ld, int rows, const int32_t* __restrict__ offsets,
                                                      int max_len, ClK K, ClWs W, float* __restrict__ plane, int32_t* __restrict__ info)
{
    __shared__ long long best[CL_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, H = K.H;
    long long o0;
    int n;
    if (!cl_scan(offsets, b, rows, max_len, &o0, &n)) return;
    long long key = -1;
    for (int h = tid; h < H; h += CL_T)
        if (W.hyp[(size_t)b * H + h].w != 0.0f) {
            const long long k = lpd_clean_choice_key(W.scores[(size_t)b * H + h], h);
            key = k > key ? k : key;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long other = __shfl_xor(key, o, 64);
        key = other > key ? other : key;
    }
    if (lane == 0) best[wave] = key;
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < CL_WAVES; ++w) key = best[w] > key ? best[w] : key;
    if (key < 0) return;      // no valid hypothesis: info (n_live, -1, 0, 0) and the zero plane stand
    const int S = (int)(key >> 10), h = LPD_CLEAN_MAX_H - 1 - (int)(key & (LPD_CLEAN_MAX_H - 1));
    info[4 * b + 2] = S;
    if (S < K.min_inliers) return;      // no road either; the best S is reported
    const float4 P = W.hyp[(size_t)b * H + h];
    const LpdCleanRows d = lpd_clean_draw((uint32_t)h, (uint32_t)b, (uint32_t)n, K.seed_lo, K.seed_hi);
    const float* s = points + ((size_t)o0 + d.i[0]) * ld;
    W.sel[b] = ClSel{P.x, P.y, P.z, s[0], s[1], s[2], 1, 0};
    plane[4 * b + 0] = P.x;
    plane[4 * b + 1] = P.y;
    plane[4 * b + 2] = P.z;
    info[4 * b + 1] = h;
    info[4 * b + 3] = S;
}

__global__ __launch_bounds__(CL_T) void moments_kernel(const float* __restrict__ points, int ld, int rows, const int32_t* __restrict__ offsets,
                                                       int max_len, ClK K, const ClSel* __restrict__ sel, unsigned long long* __restrict__ sums)
{
    __shared__ long long part[CL_WAVES][9];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = blockIdx.x * CL_CH;
    long long o0;
    int n;
    if (!cl_scan(offsets, b, rows, max_len, &o0, &n) || c0 >= n) return;
    const ClSel s = sel[b];
    if (s.status != 1) return;
    const ClRows r = cl_load(points + (size_t)o0 * ld, ld, n, c0, tid, K);
    long long a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < CL_R; ++k)
        if (lpd_clean_inlier(lpd_clean_residual(r.x[k], r.y[k], r.z[k], s.a, s.b, s.c), K.tau)) {
            const long long X = lpd_clean_quant(r.x[k], s.ox), Y = lpd_clean_quant(r.y[k], s.oy), Z = lpd_clean_quant(r.z[k], s.oz);
            a[0] += 1; a[1] += X; a[2] += Y; a[3] += Z;
            a[4] += X * X; a[5] += X * Y; a[6] += Y * Y; a[7] += X * Z; a[8] += Y * Z;
        }
#pragma unroll
    for (int j = 0; j < 9; ++j) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a[j] += __shfl_xor(a[j], o, 64);
        if (lane == 0) part[wave][j] = a[j];
    }
    __syncthreads();
    if (tid < 9) {
        long long t = part[0][tid];
        for (int w = 1; w < CL_WAVES; ++w) t += part[w][tid];
        if (t) atomicAdd(&sums[16 * b + tid], (unsigned long long)t);      // two's complement: the wrapped sum is the signed sum
    }
}

__global__ void solve_kernel(int B, ClK K, ClWs W, float* __restrict__ plane, int32_t* __restrict__ info)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    ClSel s = W.sel[b];
    if (s.status != 1) return;
    int64_t S[9];
    for (int j = 0; j < 9; ++j) S[j] = (int64_t)W.sums[16 * b + j];
    float abc[3];
    if (!lpd_clean_solve(S, s.ox, s.oy, s.oz, K.slope2, abc)) return;      // the plane of h* stands, and so does info[3] = S(h*)
    s.a = abc[0]; s.b = abc[1]; s.c = abc[2];
    s.status = 2;
    W.sel[b] = s;
    plane[4 * b + 0] = abc[0];
    plane[4 * b + 1] = abc[1];
    plane[4 * b + 2] = abc[2];
    info[4 * b + 3] = 0;      // counted again by recount_kernel
}

__global__ __launch_bounds__(CL_T) void recount_kernel(const float* __restrict__ points, int ld, int rows, const int32_t* __restrict__ offsets,
                                                       int max_len, ClK K, const ClSel* __restrict__ sel, int32_t* __restrict__ info)
{
    __shared__ int cnt;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int c0 = blockIdx.x * CL_CH;
    long long o0;
    int n;
    if (!cl_scan(offsets, b, rows, max_len, &o0, &n) || c0 >= n) return;
    const ClSel s = sel[b];
    if (s.status != 2) return;
    if (tid == 0) cnt = 0;
    const ClRows r = cl_load(points + (size_t)o0 * ld, ld, n, c0, tid, K);
    int c = 0;
#pragma unroll
    for (int k = 0; k < CL_R; ++k)
        c += __popcll(__ballot(lpd_clean_inlier(lpd_clean_residual(r.x[k], r.y[k], r.z[k], s.a, s.b, s.c), K.tau)));
    __syncthreads();
    if (lane == 0 && c) atomicAdd(&cnt, c);
    __syncthreads();
    if (tid == 0 && cnt) atomicAdd(&info[4 * b + 3], cnt);
}

// counts[b * chunks + chunk] (count) / the kept rows at their places, out_offsets and the mask (fill)
template <bool FILL>
__global__ __launch_bounds__(CL_T) void clean_kernel(const float* __restrict__ points, int ld, int rows, const int32_t* __restrict__ offsets,
                                                     int max_len, int B, ClK K, const float* __restrict__ plane, const int32_t* __restrict__ info,
                                                     int32_t* __restrict__ counts, const int32_t* __restrict__ block_off, float* __restrict__ out,
                                                     int32_t* __restrict__ out_offsets, unsigned char* __restrict__ mask)
{
    __shared__ int wcnt[CL_R * CL_WAVES];      // kept rows of (slot k, wave w) at [k * CL_WAVES + w]: the order of the rows
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunks = gridDim.x, blk = b * chunks + blockIdx.x;
    const int c0 = blockIdx.x * CL_CH;
    if (FILL && blockIdx.x == 0 && tid == 0) {
        out_offsets[b] = block_off[blk];      // the base of the scan's first chunk
        if (b == 0) out_offsets[B] = block_off[B * chunks];
    }
    long long o0;
    int n;
    if (!cl_scan(offsets, b, rows, max_len, &o0, &n) || c0 >= n) {
        if (!FILL && tid == 0) counts[blk] = 0;
        return;
    }
    const bool road = info && plane && info[4 * b + 1] >= 0;
    const float pa = road ? plane[4 * b + 0] : 0.0f, pb = road ? plane[4 * b + 1] : 0.0f, pc = road ? plane[4 * b + 2] : 0.0f;
    const ClRows r = cl_load(points + (size_t)o0 * ld, ld, n, c0, tid, K);
    bool keep[CL_R];
    unsigned long long m[CL_R];
#pragma unroll
    for (int k = 0; k < CL_R; ++k) {
        keep[k] = r.live[k] && !(road && lpd_clean_removed(lpd_clean_residual(r.x[k], r.y[k], r.z[k], pa, pb, pc), K.clearance));
        m[k] = __ballot(keep[k]);
        if (lane == 0) wcnt[k * CL_WAVES + wave] = __popcll(m[k]);
    }
    __syncthreads();
    if (!FILL) {
        if (tid == 0) {
            int t = 0;
            for (int j = 0; j < CL_R * CL_WAVES; ++j) t += wcnt[j];
            counts[blk] = t;
        }
        return;
    }
    const long long base = block_off[blk];
    const unsigned long long below = (1ull << lane) - 1ull;
    int front = 0;
#pragma unroll
    for (int k = 0; k < CL_R; ++k) {
        int mine = front;
        for (int w = 0; w < CL_WAVES; ++w) {
            const int v = wcnt[k * CL_WAVES + w];
            if (w < wave) mine += v;
            front += v;
        }
        const int i = c0 + k * CL_T + tid;
        if (keep[k]) {
            const long long at = base + mine + __popcll(m[k] & below);
            if (at >= 0 && at < rows) {      // a block_off that is not the scan of the counts cannot write outside out [rows][3]
                float* o = out + (size_t)at * 3;
                o[0] = r.x[k]; o[1] = r.y[k]; o[2] = r.z[k];
            }
        }
        if (mask && i < n) mask[(size_t)o0 + i] = keep[k] ? 1 : 0;
    }
}

int clean_check(const char* name, const float* points, int ld, int rows, const int32_t* offsets, int B, int max_len, const LpdCleanParams* p, ClK* K)
{
    LPD_CHECK_ARG(points && offsets && p, "%s: null pointer", name);
    LPD_CHECK_ARG(B >= 1 && B <= 65535 && ld >= 3 && rows >= 1, "%s: bad dims B=%d ld=%d rows=%d (1 <= B <= 65535, ld >= 3, rows >= 1)", name, B, ld,
                  rows);
    LPD_CHECK_ARG(max_len >= 1 && max_len <= LPD_CLEAN_MAX_POINTS, "%s: max_len=%d outside 1 .. 2^20", name, max_len);
    LPD_CHECK_ARG(p->r_min >= 0.0f && p->r_min <= p->r_max && p->r_max <= LPD_CLEAN_MAX_RANGE, "%s: 0 <= r_min=%g <= r_max=%g <= 512 required", name,
                  (double)p->r_min, (double)p->r_max);
    LPD_CHECK_ARG(p->z_lo == p->z_lo && p->z_hi == p->z_hi && p->seed_z_lo == p->seed_z_lo && p->seed_z_hi == p->seed_z_hi,
                  "%s: a z limit is NaN", name);
    LPD_CHECK_ARG(p->H >= 0 && p->H <= LPD_CLEAN_MAX_H, "%s: H=%d outside 0 .. %d", name, p->H, LPD_CLEAN_MAX_H);
    LPD_CHECK_ARG(lpd_clean_finite(p->tau) && p->tau >= 0.0f && lpd_clean_finite(p->min_det) && p->min_det >= 0.0f &&
                      lpd_clean_finite(p->max_slope) && p->max_slope >= 0.0f && lpd_clean_finite(p->clearance),
                  "%s: tau=%g min_det=%g max_slope=%g clearance=%g (finite; the first three >= 0)", name, (double)p->tau, (double)p->min_det,
                  (double)p->max_slope, (double)p->clearance);
    LPD_CHECK_ARG(p->min_inliers >= 0 && (p->refine == 0 || p->refine == 1), "%s: min_inliers=%d (>= 0) refine=%d (0 or 1)", name, p->min_inliers,
                  p->refine);
    *K = ClK{lpd_clean_sq(p->r_min), lpd_clean_sq(p->r_max), p->z_lo, p->z_hi, p->seed_z_lo, p->seed_z_hi, p->tau, p->min_det,
             lpd_clean_sq(p->max_slope), p->clearance, p->H, p->min_inliers, p->seed_lo, p->seed_hi};
    return LPD_OK;
}

inline int cl_chunks(int max_len) { return (max_len + CL_CH - 1) / CL_CH; }

}  // namespace

extern "C" long long lpd_road_planes_workspace_bytes(int B, int H)
{
    if (B < 1 || B > 65535 || H < 0 || H > LPD_CLEAN_MAX_H) return 0;
    return (long long)cl_ws_bytes(B, H);
}

extern "C" int lpd_road_planes(const float* points, int ld, int rows, const int32_t* offsets, int B, int max_len, const LpdCleanParams* prm,
                               float* plane, int32_t* info, void* ws, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    ClK K;
    const int rc = clean_check("lpd_road_planes", points, ld, rows, offsets, B, max_len, prm, &K);
    if (rc != LPD_OK) return rc;
    LPD_CHECK_ARG(plane && info && ws, "lpd_road_planes: null pointer");
    LPD_CHECK_ARG(((uintptr_t)ws & 15) == 0, "lpd_road_planes: the workspace must be 16-byte aligned");
    const ClWs W = cl_ws(ws, B, K.H);
    const dim3 grid(cl_chunks(max_len), B);
    hipLaunchKernelGGL(hyp_kernel, dim3(B), dim3(CL_T), 0, stream, points, ld, rows, offsets, max_len, K, W, plane, info);
    hipLaunchKernelGGL(score_kernel, grid, dim3(CL_T), 0, stream, points, ld, rows, offsets, max_len, K, (const float4*)W.hyp, W.scores, info);
    if (K.H > 0) {
        hipLaunchKernelGGL(select_kernel, dim3(B), dim3(CL_T), 0, stream, points, ld, rows, offsets, max_len, K, W, plane, info);
        if (prm->refine) {
            hipLaunchKernelGGL(moments_kernel, grid, dim3(CL_T), 0, stream, points, ld, rows, offsets, max_len, K, (const ClSel*)W.sel, W.sums);
            hipLaunchKernelGGL(solve_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, B, K, W, plane, info);
            hipLaunchKernelGGL(recount_kernel, grid, dim3(CL_T), 0, stream, points, ld, rows, offsets, max_len, K, (const ClSel*)W.sel, info);
        }
    }
    LPD_CHECK_LAUNCH("lpd_road_planes");
    return LPD_OK;
}

extern "C" int lpd_clean_count(const float* points, int ld, int rows, const int32_t* offsets, int B, int max_len, const LpdCleanParams* prm,
                               const float* plane, const int32_t* info, int32_t* counts, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    ClK K;
    const int rc = clean_check("lpd_clean_count", points, ld, rows, offsets, B, max_len, prm, &K);
    if (rc != LPD_OK) return rc;
    LPD_CHECK_ARG(counts && (plane == nullptr) == (info == nullptr), "lpd_clean_count: null pointer (plane and info go together)");
    hipLaunchKernelGGL(clean_kernel<false>, dim3(cl_chunks(max_len), B), dim3(CL_T), 0, stream, points, ld, rows, offsets, max_len, B, K, plane, info,
                       counts, (const int32_t*)nullptr, (float*)nullptr, (int32_t*)nullptr, (unsigned char*)nullptr);
    LPD_CHECK_LAUNCH("lpd_clean_count");
    return LPD_OK;
}

extern "C" int lpd_clean_fill(const float* points, int ld, int rows, const int32_t* offsets, int B, int max_len, const LpdCleanParams* prm,
                              const float* plane, const int32_t* info, const int32_t* block_off, float* out, int32_t* out_offsets,
                              unsigned char* mask, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    ClK K;
    const int rc = clean_check("lpd_clean_fill", points, ld, rows, offsets, B, max_len, prm, &K);
    if (rc != LPD_OK) return rc;
    LPD_CHECK_ARG(block_off && out && out_offsets && (plane == nullptr) == (info == nullptr),
                  "lpd_clean_fill: null pointer (plane and info go together)");
    LPD_CHECK_ARG((const void*)out != (const void*)points, "lpd_clean_fill: out must not alias points");
    hipLaunchKernelGGL(clean_kernel<true>, dim3(cl_chunks(max_len), B), dim3(CL_T), 0, stream, points, ld, rows, offsets, max_len, B, K, plane, info,
                       (int32_t*)nullptr, block_off, out, out_offsets, mask);
    LPD_CHECK_LAUNCH("lpd_clean_fill");
    return LPD_OK;
}
