// lpd_submap.hip -- raw LiDAR scans -> submaps: a ragged batch of clouds of any length (1 .. 2^20 points) becomes [B][N][3] model
// input in ONE launch.  Voxel-grid average whose cell size is searched so that the number of occupied cells lands just under N,
// filled up to exactly N with raw points, shifted to zero mean and scaled into [-1, 1].  No counterpart in the reference: its
// submaps come from an offline preprocessing step.  Definition: include/lpd_hip.h; per-point arithmetic: lpd_submap_math.h.
//
// One 1024-thread block per cloud (as lpd_morton.hip); the points are re-read from global memory / L2 in every pass:
//   box        min / max per axis                                                         1 pass
//   search     7 bisection steps over the 128 rungs; count(j) = number of distinct 30-bit Morton keys, counted with a SET in LDS
//              (atomicCAS insertion, open addressing, linear probing).  A pass is abandoned as soon as more than N keys are in.
//              An eighth pass re-fills the set at j* when the last step looked at another rung.     7-8 passes
//   rows       the set's keys are compacted, sorted (bitonic, in LDS) -- distinct keys: a deterministic order whatever the
//              insertion order was; every point finds its row by binary search and adds its quantised coordinates to the row's
//              three 64-bit integer sums and its count with LDS integer atomics: exact, so independent of the order.   1 pass
//   output     <= 4 rows per thread in registers: centroids / fill rows, fp64 mean by a fixed-order block reduction, max |d|.
// No float atomics anywhere.
//
// THE TABLE NEVER FILLS.  The distinct count is read once per block-wide trip (1024 points), between two barriers, and the pass
// stops when it exceeds N: a trip starts with at most N keys in the set and adds at most 1024, so at most N + 1024 of the
// TS = max(2 NP, 4096) slots are ever taken (NP = N rounded up to a power of two; 5120 of 8192 at N = 4096; checked by the entry
// point).  Every probe loop is bounded by TS on top of that.
//
// LDS (N = 4096): keys 16 KiB + counts 16 KiB + sums 4096 x 3 x 8 B = 96 KiB, 128 KiB in all; the 32 KiB set lives in the sums'
// space (it is dead once the keys are compacted).
#include "lpd_common.h"
#include "lpd_submap_math.h"

namespace {

constexpr int SM_T = 1024;
constexpr uint32_t SM_EMPTY = 0xffffffffu;      // keys have 30 bits

inline int sm_pow2(int N)
{
    int p = LPD_SUBMAP_MIN_N;
    while (p < N) p <<= 1;
    return p;
}
inline int sm_table(int NP) { return 2 * NP > 4096 ? 2 * NP : 4096; }
inline size_t sm_lds_bytes(int NP, int TS)
{
    const size_t big = (size_t)NP * 24 > (size_t)TS * 4 ? (size_t)NP * 24 : (size_t)TS * 4;
    return (size_t)NP * 8 + big;
}

struct SmPoint { float x, y, z; };

__device__ __forceinline__ SmPoint sm_load(const float* __restrict__ p, int ld, int i)
{
    const float* q = p + (size_t)i * ld;
    return SmPoint{q[0], q[1], q[2]};
}

// Fill the set with the keys of the cloud on the rung with scale s; -> the number of distinct keys when it is <= N, else some
// count > N (the pass was abandoned).  Called by all threads; the result is the same in all of them.
__device__ int sm_count_pass(const float* __restrict__ p, int ld, int n, float mnx, float mny, float mnz, float s, uint32_t* tab, int TS,
                             int tshift, int N, int* count)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < TS; i += SM_T) tab[i] = SM_EMPTY;
    if (tid == 0) *count = 0;
    __syncthreads();
    int c = 0;
    SmPoint nxt = tid < n ? sm_load(p, ld, tid) : SmPoint{0.0f, 0.0f, 0.0f};
    for (int base = 0; base < n; base += SM_T) {      // one trip: at most 1024 new keys
        const int i = base + tid;
        const SmPoint cur = nxt;
        if (i + SM_T < n) nxt = sm_load(p, ld, i + SM_T);      // the next trip's point is under way while this one is inserted
        if (i < n) {
            const uint32_t key = lpd_submap_key(cur.x, cur.y, cur.z, mnx, mny, mnz, s);
            uint32_t slot = (key * 2654435761u) >> tshift;
            for (int probe = 0; probe < TS; ++probe) {      // bounded: cannot spin even on a full table
                const uint32_t old = atomicCAS(&tab[slot], SM_EMPTY, key);
                if (old == SM_EMPTY) {
                    atomicAdd(count, 1);      // (one add per wave after a ballot instead: 903 us against 810 for 32 scans)
                    break;
                }
                if (old == key) break;
                slot = (slot + 1) & (uint32_t)(TS - 1);
            }
        }
        __syncthreads();
        c = *(volatile int*)count;      // read between two barriers: every thread sees the same value and takes the same branch
        __syncthreads();
        if (c > N) break;
    }
    return c;
}

__global__ __launch_bounds__(SM_T) void make_submaps_kernel(const float* __restrict__ points, int ld, const int32_t* __restrict__ offsets, int N,
                                                            int NP, int TS, int tshift, int normalize, float* __restrict__ out,
                                                            int32_t* __restrict__ info, float* __restrict__ xform, int32_t* __restrict__ counts)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_lds[];
    uint32_t* keys = reinterpret_cast<uint32_t*>(sm_lds);                          // [NP] sorted distinct keys, padded with SM_EMPTY
    int* cnt = reinterpret_cast<int*>(keys + NP);                                  // [NP] points per cell
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(cnt + NP);    // [NP][3] integer coordinate sums
    uint32_t* tab = reinterpret_cast<uint32_t*>(sums);                             // [TS] the set of the search (dead before sums is used)
    __shared__ float red[6][SM_T / 64];
    __shared__ double redd[3][SM_T / 64];
    __shared__ float box[4];       // mn_x, mn_y, mn_z, E; later mean_x, mean_y, mean_z, r
    __shared__ int s_count, s_pos;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long o0 = offsets[b], o1 = offsets[b + 1];
    float* ob = out + (size_t)b * N * 3;
    if (o0 < 0 || o1 - o0 < 1 || o1 - o0 > LPD_SUBMAP_MAX_POINTS) {
        // offsets the definition excludes (the Python wrapper rejects them on the host): a marked, zeroed cloud, no read of the points
        for (int r = tid; r < N; r += SM_T) {
            ob[3 * r] = ob[3 * r + 1] = ob[3 * r + 2] = 0.0f;
            if (counts) counts[(size_t)b * N + r] = 0;
        }
        if (tid < 4) {
            info[4 * b + tid] = tid == 0 ? -1 : 0;
            xform[4 * b + tid] = 0.0f;
        }
        return;
    }
    const int n = (int)(o1 - o0);
    const float* p = points + (size_t)o0 * ld;

    // ---- 1. box
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = tid; i < n; i += SM_T) {
        const SmPoint q = sm_load(p, ld, i);
        mn[0] = fminf(mn[0], q.x); mx[0] = fmaxf(mx[0], q.x);
        mn[1] = fminf(mn[1], q.y); mx[1] = fmaxf(mx[1], q.y);
        mn[2] = fminf(mn[2], q.z); mx[2] = fmaxf(mx[2], q.z);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn[c] = fminf(mn[c], __shfl_xor(mn[c], o, 64));
            mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], o, 64));
        }
        if (lane == 0) { red[c][wave] = mn[c]; red[3 + c][wave] = mx[c]; }
    }
    __syncthreads();
    if (tid == 0) {
        float E = 0.0f;
        for (int c = 0; c < 3; ++c) {
            float a = red[c][0], z = red[3 + c][0];
            for (int w = 1; w < SM_T / 64; ++w) { a = fminf(a, red[c][w]); z = fmaxf(z, red[3 + c][w]); }
            box[c] = a;
            E = fmaxf(E, z - a);
        }
        box[3] = E;
    }
    __syncthreads();
    const float mnx = box[0], mny = box[1], mnz = box[2], E = box[3];

    // ---- 2./3. bisection over the ladder
    int lo = -1, hi = LPD_SUBMAP_RUNGS - 1, last = -1, c = 0;
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;      // lo + hi >= 0 here
        c = sm_count_pass(p, ld, n, mnx, mny, mnz, lpd_submap_scale(mid, E), tab, TS, tshift, N, &s_count);
        last = mid;
        if (c <= N) hi = mid;
        else lo = mid;
    }
    if (last != hi) c = sm_count_pass(p, ld, n, mnx, mny, mnz, lpd_submap_scale(hi, E), tab, TS, tshift, N, &s_count);
    const int M = c < N ? c : N;      // c <= N by the search (rung 127 has at most 125 cells); the min keeps every index below in range

    // ---- 4. the set's keys, compacted and sorted
    for (int i = tid; i < NP; i += SM_T) {
        keys[i] = SM_EMPTY;
        cnt[i] = 0;
    }
    if (tid == 0) s_pos = 0;
    __syncthreads();
    for (int i = tid; i < TS; i += SM_T) {
        const uint32_t k = tab[i];
        if (k != SM_EMPTY) {
            const int pos = atomicAdd(&s_pos, 1);
            if (pos < NP) keys[pos] = k;
        }
    }
    __syncthreads();
    for (int k = 2; k <= NP; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < NP / 2; t += SM_T) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;      // the pair (i, i + j)
                const bool up = (i & k) == 0;
                const uint32_t a = keys[i], z = keys[l];
                if ((a > z) == up) {
                    keys[i] = z;
                    keys[l] = a;
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < NP * 3; i += SM_T) sums[i] = 0ull;      // the set is dead: its space becomes the sums
    __syncthreads();

    // every point -> its row (binary search; the padding sorts behind every key) -> integer sums
    {
        const float s = lpd_submap_scale(hi, E), f = lpd_submap_qscale(E);
        SmPoint nxt = tid < n ? sm_load(p, ld, tid) : SmPoint{0.0f, 0.0f, 0.0f};
        for (int i = tid; i < n; i += SM_T) {
            const SmPoint cur = nxt;
            if (i + SM_T < n) nxt = sm_load(p, ld, i + SM_T);
            const uint32_t key = lpd_submap_key(cur.x, cur.y, cur.z, mnx, mny, mnz, s);
            int pos = 0;
            for (int step = NP >> 1; step > 0; step >>= 1)
                if (keys[pos + step - 1] < key) pos += step;      // pos + step - 1 <= NP - 2
            if (pos < M && keys[pos] == key) {
                atomicAdd(&sums[3 * pos + 0], (unsigned long long)lpd_submap_quant(cur.x, mnx, f));
                atomicAdd(&sums[3 * pos + 1], (unsigned long long)lpd_submap_quant(cur.y, mny, f));
                atomicAdd(&sums[3 * pos + 2], (unsigned long long)lpd_submap_quant(cur.z, mnz, f));
                atomicAdd(&cnt[pos], 1);
            }
        }
    }
    __syncthreads();

    // ---- 4./5. rows: thread t holds rows t, t + 1024, ...
    constexpr int RPT = LPD_SUBMAP_MAX_N / SM_T;
    const float qstep = lpd_submap_qstep(E);
    float row[RPT][3];
    double dsum[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int r = tid + k * SM_T;
        row[k][0] = row[k][1] = row[k][2] = 0.0f;
        if (r < N) {
            int m = 0;
            if (r < M) {
                m = cnt[r];
                if (m > 0) {
                    row[k][0] = lpd_submap_centroid(sums[3 * r + 0], m, mnx, qstep);
                    row[k][1] = lpd_submap_centroid(sums[3 * r + 1], m, mny, qstep);
                    row[k][2] = lpd_submap_centroid(sums[3 * r + 2], m, mnz, qstep);
                }
            } else {
                const SmPoint q = sm_load(p, ld, (int)lpd_submap_fill_index(r - M, n, N - M));      // < n: (2 p + 1) < 2 (N - M)
                row[k][0] = q.x; row[k][1] = q.y; row[k][2] = q.z;
            }
            if (counts) counts[(size_t)b * N + r] = m;
            dsum[0] += (double)row[k][0];
            dsum[1] += (double)row[k][1];
            dsum[2] += (double)row[k][2];
        }
    }
    if (tid == 0) {
        info[4 * b + 0] = hi;
        info[4 * b + 1] = M;
        info[4 * b + 2] = n;
        info[4 * b + 3] = 0;
    }
    if (!normalize) {
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const int r = tid + k * SM_T;
            if (r < N) { ob[3 * r] = row[k][0]; ob[3 * r + 1] = row[k][1]; ob[3 * r + 2] = row[k][2]; }
        }
        if (tid < 4) xform[4 * b + tid] = tid == 3 ? 1.0f : 0.0f;      // the identity: out = (row - 0) * 1
        return;
    }

    // ---- 6. mean: fp64, fixed order (thread: its rows ascending; wave: xor tree; block: waves ascending)
#pragma unroll
    for (int c2 = 0; c2 < 3; ++c2) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dsum[c2] += __shfl_xor(dsum[c2], o, 64);
        if (lane == 0) redd[c2][wave] = dsum[c2];
    }
    __syncthreads();
    if (tid < 3) {
        double a = redd[tid][0];
        for (int w = 1; w < SM_T / 64; ++w) a += redd[tid][w];
        box[tid] = (float)(a / (double)N);
    }
    __syncthreads();
    const float mean[3] = {box[0], box[1], box[2]};
    float rmax = 0.0f;
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int r = tid + k * SM_T;
#pragma unroll
        for (int c2 = 0; c2 < 3; ++c2) {
            row[k][c2] -= mean[c2];
            if (r < N) rmax = fmaxf(rmax, fabsf(row[k][c2]));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rmax = fmaxf(rmax, __shfl_xor(rmax, o, 64));
    if (lane == 0) red[0][wave] = rmax;
    __syncthreads();
    if (tid == 0) {
        float a = red[0][0];
        for (int w = 1; w < SM_T / 64; ++w) a = fmaxf(a, red[0][w]);
        box[3] = a;
    }
    __syncthreads();
    const float rr = box[3], inv = rr > 0.0f ? 1.0f / rr : 0.0f;
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int r = tid + k * SM_T;
        if (r < N) {
            ob[3 * r + 0] = rr > 0.0f ? row[k][0] * inv : 0.0f;
            ob[3 * r + 1] = rr > 0.0f ? row[k][1] * inv : 0.0f;
            ob[3 * r + 2] = rr > 0.0f ? row[k][2] * inv : 0.0f;
        }
    }
    if (tid < 4) xform[4 * b + tid] = box[tid];
}

}  // namespace

extern "C" int lpd_make_submaps(const float* points, int ld, const int32_t* offsets, int B, int N, int normalize, float* out, int32_t* info,
                                float* xform, int32_t* counts, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(points && offsets && out && info && xform, "lpd_make_submaps: null pointer");
    LPD_CHECK_ARG(B > 0 && ld >= 3, "lpd_make_submaps: bad dims B=%d ld=%d (B > 0, ld >= 3)", B, ld);
    LPD_CHECK_ARG(N >= LPD_SUBMAP_MIN_N, "lpd_make_submaps: N=%d < %d (the search over the ladder needs N >= %d)", N, LPD_SUBMAP_MIN_N,
                  LPD_SUBMAP_MIN_N);
    LPD_CHECK_ARG(normalize == 0 || normalize == 1, "lpd_make_submaps: normalize=%d (0 or 1)", normalize);
    LPD_CHECK_ARG((const void*)out != (const void*)points, "lpd_make_submaps: out must not alias points");
    if (N > LPD_SUBMAP_MAX_N) {
        lpd_set_error("lpd_make_submaps: N=%d > %d unsupported", N, LPD_SUBMAP_MAX_N);
        return LPD_ERR_UNSUPPORTED;
    }
    const int NP = sm_pow2(N), TS = sm_table(NP);
    int tshift = 32;
    while ((1 << (32 - tshift)) < TS) --tshift;
    // the set can never fill: at most N + 1024 keys are in when a pass is abandoned
    LPD_CHECK_ARG(TS == (1 << (32 - tshift)) && TS > N + SM_T, "lpd_make_submaps: table of %d slots for N=%d", TS, N);
    const size_t lds = sm_lds_bytes(NP, TS);
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)make_submaps_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(make_submaps_kernel, dim3(B), dim3(SM_T), lds, stream, points, ld, offsets, N, NP, TS, tshift, normalize, out, info, xform,
                       counts);
    LPD_CHECK_LAUNCH("lpd_make_submaps");
    return LPD_OK;
}
