// lpd_tuples.hip -- the input side of the training loop on the device: lpd_sample_items draws distinct items uniformly from a union
// of item lists (or from its complement), lpd_gather_tuples writes the model's [B][N][3] input from the resident cloud table, with
// the reference's rotation about z and per-point jitter (util/data.py:56-101, loading_pointclouds.py:50-85 on the host there).
// Definitions: include/lpd_hip.h; integer and per-point arithmetic: lpd_tuple_math.h.
//
// lpd_sample_items, one 1024-thread workgroup per row:
//   bitmap   membership of [0, T) in LDS: ceil(T / 32) words, set with LDS atomicOr from the row's lists and extras (items and list
//            numbers outside their range are skipped before anything is addressed with them); inverted in place for the complement
//   scan     popcount per word, block-wide exclusive scan (thread: a contiguous run of words; wave: shuffles; block: 16 wave totals)
//   draw     sample j -> p = perm(j, c, seed, row) -> the word with scan[w] <= p < scan[w] + popcount (binary search) -> the
//            (p - scan[w])-th set bit of that word
// Integer arithmetic only, no atomics on global memory: the same bits in every launch.
// LDS: 2 x ceil(T / 32) words + 16 wave totals; 64 KiB + 64 B at T = 262144.
#include "lpd_common.h"
#include "lpd_tuple_math.h"

namespace {

constexpr int TP_T = 1024;            // threads of a sampling workgroup
constexpr int TP_WAVES = TP_T / 64;

__global__ __launch_bounds__(TP_T) void sample_items_kernel(const int32_t* __restrict__ off, const int32_t* __restrict__ idx, int n_lists, int nnz,
                                                            int T, const int32_t* __restrict__ lists, int L, const int32_t* __restrict__ extra,
                                                            int X, int invert, int m, unsigned long long seed, int32_t* __restrict__ out,
                                                            int32_t* __restrict__ count)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char tp_lds[];
    const int W = (T + 31) >> 5;
    uint32_t* bm = reinterpret_cast<uint32_t*>(tp_lds);      // [W] membership
    uint32_t* sc = bm + W;                                   // [W] exclusive scan of the popcounts
    uint32_t* wtot = sc + W;                                 // [TP_WAVES]
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int w = tid; w < W; w += TP_T) bm[w] = 0u;
    __syncthreads();
    for (int l = 0; l < L; ++l) {
        const int ln = lists[(size_t)r * L + l];      // uniform over the block
        if (ln < 0 || ln >= n_lists) continue;
        int a = off[ln], e = off[ln + 1];
        if (a < 0) a = 0;
        if (e > nnz) e = nnz;
        for (int k = a + tid; k < e; k += TP_T) {
            const int it = idx[k];
            if (it >= 0 && it < T) atomicOr(&bm[it >> 5], 1u << (it & 31));
        }
    }
    if (tid < X) {
        const int it = extra[(size_t)r * X + tid];
        if (it >= 0 && it < T) atomicOr(&bm[it >> 5], 1u << (it & 31));
    }
    __syncthreads();

    // popcounts and their exclusive scan; thread t owns words t * per .. t * per + per - 1
    const int per = (W + TP_T - 1) / TP_T;      // <= 8
    const int w0 = tid * per;
    const uint32_t tail = (T & 31) ? ((1u << (T & 31)) - 1u) : 0xffffffffu;      // the bits of the last word that are items
    uint32_t mine = 0;
    for (int i = 0; i < per; ++i) {
        const int w = w0 + i;
        if (w < W) {
            uint32_t v = bm[w];
            if (invert) {
                v = ~v;
                if (w == W - 1) v &= tail;
                bm[w] = v;
            }
            mine += (uint32_t)__popc(v);
        }
    }
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t before = 0, c = 0;
#pragma unroll
    for (int i = 0; i < TP_WAVES; ++i) {
        const uint32_t t = wtot[i];
        if (i < wave) before += t;
        c += t;
    }
    uint32_t run = before + incl - mine;
    for (int i = 0; i < per; ++i) {
        const int w = w0 + i;
        if (w < W) {
            sc[w] = run;
            run += (uint32_t)__popc(bm[w]);
        }
    }
    __syncthreads();
    if (tid == 0) count[r] = (int32_t)c;

    const LpdPermKeys K = lpd_tuple_perm_keys(seed, (uint32_t)r);
    const int h = lpd_tuple_perm_half_bits(c);
    for (int j = tid; j < m; j += TP_T) {
        int32_t item = -1;
        if ((uint32_t)j < c) {
            const uint32_t p = lpd_tuple_perm_with((uint32_t)j, c, K, h);
            int lo = 0, hi = W;      // first word with sc > p; sc[0] = 0 <= p, so lo >= 1 at the end
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sc[mid] <= p) lo = mid + 1;
                else hi = mid;
            }
            const int w = lo - 1;      // the LAST word with sc <= p: the words behind it up to lo have no bits, it has one
            item = (int32_t)((uint32_t)w * 32u + lpd_tuple_select_bit(bm[w], p - sc[w]));
        }
        out[(size_t)r * m + j] = item;
    }
}

// ---- gather: thread = four points (three float4) when VEC, one point otherwise; blockIdx.y = slot in the batch
template <bool VEC>
__global__ __launch_bounds__(256) void gather_tuples_kernel(const float* __restrict__ table, int T, int N, const int32_t* __restrict__ items,
                                                            const float* __restrict__ rot, float sigma, float clip, uint32_t seed_lo,
                                                            uint32_t seed_hi, float* __restrict__ out)
{
    constexpr int PTS = VEC ? 4 : 1;
    const int b = blockIdx.y;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;      // group of PTS points
    if ((long long)g * PTS >= N) return;
    const int item = items[b];
    float* o = out + ((size_t)b * N + (size_t)g * PTS) * 3;
    float v[PTS * 3];
    if (item < 0 || item >= T) {      // never read
#pragma unroll
        for (int i = 0; i < PTS * 3; ++i) v[i] = 0.0f;
    } else {
        const float* p = table + ((size_t)item * N + (size_t)g * PTS) * 3;
        if constexpr (VEC) {
            const float4* p4 = reinterpret_cast<const float4*>(p);
            const float4 a = p4[0], bb = p4[1], cc = p4[2];
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
            v[4] = bb.x; v[5] = bb.y; v[6] = bb.z; v[7] = bb.w;
            v[8] = cc.x; v[9] = cc.y; v[10] = cc.z; v[11] = cc.w;
        } else {
            v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
        }
        if (rot) {      // pc @ R of the reference: x' = x c + y s, y' = -x s + y c
            const float c = rot[2 * b], s = rot[2 * b + 1];
#pragma unroll
            for (int i = 0; i < PTS; ++i) {
                const float x = v[3 * i], y = v[3 * i + 1];
                v[3 * i] = x * c + y * s;
                v[3 * i + 1] = -x * s + y * c;
            }
        }
        if (sigma != 0.0f) {
#pragma unroll
            for (int i = 0; i < PTS; ++i) {
                float d[3];
                lpd_tuple_jitter((uint32_t)(g * PTS + i), (uint32_t)b, seed_lo, seed_hi, sigma, clip, d);
                v[3 * i] += d[0];
                v[3 * i + 1] += d[1];
                v[3 * i + 2] += d[2];
            }
        }
    }
    if constexpr (VEC) {
        float4* o4 = reinterpret_cast<float4*>(o);
        o4[0] = make_float4(v[0], v[1], v[2], v[3]);
        o4[1] = make_float4(v[4], v[5], v[6], v[7]);
        o4[2] = make_float4(v[8], v[9], v[10], v[11]);
    } else {
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    }
}

}  // namespace

extern "C" int lpd_sample_items(const int32_t* off, const int32_t* idx, int n_lists, int nnz, int T, const int32_t* lists, int L,
                                const int32_t* extra, int X, int R, int invert, int m, unsigned long long seed, int32_t* out, int32_t* count,
                                void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(off && out && count, "lpd_sample_items: null pointer");
    LPD_CHECK_ARG(n_lists >= 0 && nnz >= 0 && (nnz == 0 || idx), "lpd_sample_items: bad lists n_lists=%d nnz=%d", n_lists, nnz);
    LPD_CHECK_ARG(T >= 1 && T <= LPD_TUPLE_MAX_ITEMS, "lpd_sample_items: T=%d outside 1 .. %d", T, LPD_TUPLE_MAX_ITEMS);
    LPD_CHECK_ARG(m >= 1 && m <= LPD_TUPLE_MAX_SAMPLES, "lpd_sample_items: m=%d outside 1 .. %d", m, LPD_TUPLE_MAX_SAMPLES);
    LPD_CHECK_ARG(L >= 0 && L <= LPD_TUPLE_MAX_LISTS && (L == 0 || lists), "lpd_sample_items: L=%d outside 0 .. %d (or lists is null)", L,
                  LPD_TUPLE_MAX_LISTS);
    LPD_CHECK_ARG(X >= 0 && X <= LPD_TUPLE_MAX_LISTS && (X == 0 || extra), "lpd_sample_items: X=%d outside 0 .. %d (or extra is null)", X,
                  LPD_TUPLE_MAX_LISTS);
    LPD_CHECK_ARG(R >= 1 && R <= LPD_TUPLE_MAX_ROWS, "lpd_sample_items: R=%d outside 1 .. %d", R, LPD_TUPLE_MAX_ROWS);
    LPD_CHECK_ARG(invert == 0 || invert == 1, "lpd_sample_items: invert=%d (0 or 1)", invert);
    const int W = (T + 31) / 32;
    const size_t lds = ((size_t)2 * W + TP_WAVES) * sizeof(uint32_t);
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)sample_items_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(sample_items_kernel, dim3(R), dim3(TP_T), lds, stream, off, idx, n_lists, nnz, T, lists, L, extra, X, invert, m, seed,
                       out, count);
    LPD_CHECK_LAUNCH("lpd_sample_items");
    return LPD_OK;
}

extern "C" int lpd_gather_tuples(const float* table, int T, int N, const int32_t* items, int B, const float* rot, float sigma, float clip,
                                 unsigned long long seed, float* out, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(table && items && out, "lpd_gather_tuples: null pointer");
    LPD_CHECK_ARG(T >= 1 && N >= 1 && N <= (1 << 20), "lpd_gather_tuples: bad dims T=%d N=%d (T >= 1, 1 <= N <= 2^20)", T, N);
    LPD_CHECK_ARG(B >= 1 && B <= LPD_TUPLE_MAX_ROWS, "lpd_gather_tuples: B=%d outside 1 .. %d", B, LPD_TUPLE_MAX_ROWS);
    LPD_CHECK_ARG(sigma >= 0.0f && clip > 0.0f, "lpd_gather_tuples: sigma=%g clip=%g (sigma >= 0, clip > 0)", (double)sigma, (double)clip);
    LPD_CHECK_ARG((const void*)out != (const void*)table, "lpd_gather_tuples: out must not alias table");
    const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
    // four points = 48 bytes = three 16-byte words: every cloud row starts on a 16-byte boundary when N % 4 == 0 and the bases do
    const bool vec = N % 4 == 0 && ((uintptr_t)table & 15) == 0 && ((uintptr_t)out & 15) == 0;
    if (vec) {
        const int groups = N / 4;
        hipLaunchKernelGGL(gather_tuples_kernel<true>, dim3((groups + 255) / 256, B), dim3(256), 0, stream, table, T, N, items, rot, sigma, clip,
                           lo, hi, out);
    } else {
        hipLaunchKernelGGL(gather_tuples_kernel<false>, dim3((N + 255) / 256, B), dim3(256), 0, stream, table, T, N, items, rot, sigma, clip, lo,
                           hi, out);
    }
    LPD_CHECK_LAUNCH("lpd_gather_tuples");
    return LPD_OK;
}
