// lpd_align.hip -- geometric verification of retrieved places: correlative scan matching of (query, candidate) submap pairs over yaw
// and a window of cell shifts, on bird's-eye occupancy bitmaps with a few height layers.  What stands between lpd_recall_pairs'
// topk_idx and a loop-closure constraint, without copying a cloud back.  Definition: include/lpd_hip.h; arithmetic: lpd_align_math.h.
//
// align_kernel, AL_T = 256 threads = 4 waves, one workgroup per (pair, slice of the hypotheses):
//   B's bitmap    built once per workgroup by all threads with LDS atomicOr: [layer][176 rows] of 16 bytes (11 KiB): the 128 rows of
//                 the grid with 16 zero rows in front and 32 behind, so that no read of the scoring loop needs a range test
//   A's points    N <= 4096: what every hypothesis shares of a point -- the scaled (px, py) and the layer, 9 bytes -- is computed once
//                 per workgroup and kept in dynamic LDS (36 KiB at N = 4096).  Larger clouds are read from memory by every hypothesis.
//   A's bitmaps   one per wave, [layer][128 rows] of 16 bytes (8 KiB each): wave w of slice g takes the hypotheses h0 + 4 * it + w and
//                 rasterises A under its own (cos, sin), 64 points a step
//   scoring       THE LANES ARE THE ROWS.  A (layer, half) block is 64 rows, lane = row: the lane's A row is shifted by dx ONCE (dx is
//                 wave-uniform: three VALU operations a word), then for every dy the B row iy + dy is one 16-byte LDS read at
//                 consecutive slots (conflict-free) and the lane adds popcount(shifted & b) to acc[dy]: 4 AND + 4 v_bcnt.  The kernel
//                 is built for NDY = 1, 3, 9, 17 and 33 rows of dy (the smallest that holds 2S + 1), so that a block's reads are
//                 issued together with no branch between them.  Per dx the sums are reduced over the wave (DPP, no LDS), two 16-bit
//                 sums to a word (a score is at most N <= 16384), and compared as packed keys.  Blocks of A that are empty in all 64
//                 rows are skipped (a ballot).
//                 The other layout -- lanes take the (dy, dx) shifts, the A row a broadcast -- needs a per-lane shift of every A row
//                 (5 selects + 4 funnel shifts) for every (row, dy, dx) and leaves 31 of 64 lanes idle in the last of five passes at
//                 S = 8; this one shifts once per (row, dx) and fills every lane for every S.
//   choice        key = score << 36 | (2^21 - 1 - candidate number) << 15 | nA (lpd_align_key): an integer maximum, the same in any
//                 order.  waves -> LDS -> the workgroup's key.  One slice (G = 1): the workgroup writes `best`.  G > 1: it stores its
//                 key at ws[pair][slice] (a plain store, nothing to clear) and align_finish_kernel takes the maximum in slice order.
// The split: a pair's H hypotheses are cut into G = min(ceil(H / 4), max(1, 512 / P)) slices, so that a single query's 25 candidates
// fill the chip (500 workgroups) and a batch of 512 pairs or more runs one workgroup a pair with no second launch.
// No float atomics anywhere; LDS integer atomicOr / atomicAdd only: the same bits in every launch.
//
// Registers / LDS: NDY accumulators and the rows in flight (88 VGPRs at NDY = 17, 138 at 33, no scratch).  43 KiB of static LDS a
// workgroup, and with the staged points of N = 4096 another 36 KiB: 79 KiB, two workgroups on a CU's 160 KiB (three when N > 4096).
// The measurements, and what was tried and dropped: DESIGN.md 13h, profiles/align_bench.txt.
#include <math.h>

#include "lpd_common.h"
#include "lpd_align_math.h"

namespace {

constexpr int AL_T = 256;
constexpr int AL_WAVES = AL_T / 64;
constexpr int AL_G = LPD_ALIGN_GRID;                 // 128
// B's bitmap has AL_PAD = 16 zero rows in front of row 0 (dy >= -16) and AL_TAIL = 32 behind row 127: the scoring loop reads NDY rows
// from row + AL_PAD - S on, and NDY can exceed 2S + 1 (S = 9 reads 33 rows: up to row 127 + 16 - 9 + 32 = 166 of 176)
constexpr int AL_PAD = LPD_ALIGN_MAX_S;
constexpr int AL_TAIL = 2 * LPD_ALIGN_MAX_S;
constexpr int AL_BROWS = AL_G + AL_PAD + AL_TAIL;    // 176
constexpr int AL_LMAX = LPD_ALIGN_MAX_LAYERS;
constexpr int AL_SPAN = LPD_ALIGN_SPAN;
constexpr int AL_TARGET_WGS = 512;
constexpr int AL_STAGE_N = 4096;                     // clouds up to this size are kept in LDS (9 bytes a point: 36 KiB, two workgroups a CU)
static_assert(AL_G == 128 && AL_SPAN == 2 * LPD_ALIGN_MAX_S + 1, "a row is four words; dy + S and dx + S are below the radix");
static_assert(LPD_ALIGN_MAX_H * AL_SPAN * AL_SPAN < (1 << 21) && LPD_ALIGN_MAX_POINTS < (1 << 15), "the key's fields");

struct AlSlot { unsigned long long key; int32_t nB, pad; };      // ws[pair][slice]

struct AlK {
    int TA, TB, N, P, R, H, S, layers, G, hs;      // G slices of hs hypotheses
    int staged;                                    // A's points are kept in the dynamic LDS
    float inv_cell, z0, inv_zcell;
};

// slices per pair and hypotheses per slice
inline void al_split(int P, int H, int* G, int* hs)
{
    int g = AL_TARGET_WGS / P;
    const int gmax = (H + AL_WAVES - 1) / AL_WAVES;
    g = g < 1 ? 1 : (g > gmax ? gmax : g);
    *hs = (H + g - 1) / g;
    *G = (H + *hs - 1) / *hs;      // no empty slice
}

// The sum over the wave, the same in every lane.  Four DPP steps (lane ^ 1, lane ^ 2, the mirrored half row, the mirrored row) leave
// every lane with the sum of its row of 16; the four rows are read as scalars.  No LDS traffic: __shfl_xor compiles to ds_bpermute,
// six dependent ones a sum, and a hypothesis at S = 8 takes 17 x 9 sums.
__device__ __forceinline__ int al_wave_sum(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);       // quad_perm [1, 0, 3, 2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);       // quad_perm [2, 3, 0, 1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);      // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false);      // row_mirror
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}

__device__ __forceinline__ bool al_pair_ok(const int32_t* __restrict__ pairs, int p, int TA, int TB, int* ra, int* rb)
{
    *ra = pairs[2 * p];
    *rb = pairs[2 * p + 1];
    return *ra >= 0 && *ra < TA && *rb >= 0 && *rb < TB;
}

__device__ __forceinline__ void al_write_missing(int32_t* __restrict__ b)
{
    b[0] = -1;
#pragma unroll
    for (int j = 1; j < 8; ++j) b[j] = 0;
}

// NDY = 1, 3, 9, 17 or 33: the dy rows the scoring loop reads, the smallest of them that holds 2S + 1
template <int NDY>
__global__ __launch_bounds__(AL_T) void align_kernel(const float* __restrict__ A,const float* __restrict__ scaleA, const float* __restrict__ B,
                                                     const float* __restrict__ scaleB, const int32_t* __restrict__ pairs,
                                                     const float* __restrict__ rot, const int32_t* __restrict__ first,
                                                     const float* __restrict__ t0, AlK K, int32_t* __restrict__ best,
                                                     int32_t* __restrict__ yaw_scores, AlSlot* __restrict__ ws)
{
    __shared__ uint4 Bp[AL_LMAX * AL_BROWS];
    __shared__ uint4 Aw[AL_WAVES][AL_LMAX * AL_G];
    __shared__ unsigned long long wkey[AL_WAVES];
    __shared__ int nB_s;
    extern __shared__ __align__(16) unsigned char al_dyn[];      // staged: float2 [N], then N layer bytes
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x / K.G, g = blockIdx.x - p * K.G;
    const int L = K.layers, S = K.S, N = K.N, twoS = 2 * S;
    const int h0 = g * K.hs, h1 = h0 + K.hs < K.H ? h0 + K.hs : K.H;
    int ra, rb;
    if (!al_pair_ok(pairs, p, K.TA, K.TB, &ra, &rb)) {      // uniform over the workgroup: nothing of the tables is read
        if (yaw_scores)
            for (int h = h0 + tid; h < h1; h += AL_T) yaw_scores[(size_t)p * K.H + h] = 0;
        if (K.G == 1 && tid == 0) al_write_missing(best + 8 * (size_t)p);      // G > 1: align_finish_kernel writes it
        return;
    }
    // ---- B's bitmap ----
    for (int i = tid; i < L * AL_BROWS; i += AL_T) Bp[i] = make_uint4(0u, 0u, 0u, 0u);
    if (tid == 0) nB_s = 0;
    __syncthreads();
    {
        const float* pb = B + (size_t)rb * N * 3;
        const float sc = scaleB ? scaleB[rb] : 1.0f;
        uint32_t* bw = (uint32_t*)Bp;
        for (int i = tid; i < N; i += AL_T) {
            const LpdAlignCell c = lpd_align_cell_b(pb[3 * i], pb[3 * i + 1], pb[3 * i + 2], sc, K.inv_cell, K.z0, K.inv_zcell, L);
            if (c.valid) atomicOr(&bw[((c.iz * AL_BROWS + c.iy + AL_PAD) << 2) + (c.ix >> 5)], 1u << (c.ix & 31));
        }
    }
    __syncthreads();
    {
        int n = 0;
        for (int i = tid; i < L * AL_BROWS; i += AL_T) {
            const uint4 b = Bp[i];
            n += __popc(b.x) + __popc(b.y) + __popc(b.z) + __popc(b.w);
        }
        n = al_wave_sum(n);
        if (lane == 0 && n) atomicAdd(&nB_s, n);
    }
    // ---- the hypotheses of this slice, four at a time ----
    const float* pa = A + (size_t)ra * N * 3;
    const float sa = scaleA ? scaleA[ra] : 1.0f;
    const bool has_t0 = t0 != nullptr;
    const float t0x = has_t0 ? t0[2 * (size_t)p] : 0.0f, t0y = has_t0 ? t0[2 * (size_t)p + 1] : 0.0f;
    const int32_t f0 = first ? first[p] : 0;
    // A's points, what every hypothesis shares of them: (px, py) and the layer, 9 bytes a point.  A point without a layer (or not
    // finite) becomes (NaN, NaN): outside the grid under every hypothesis.
    float2* sp = (float2*)al_dyn;
    unsigned char* sl = al_dyn + (size_t)N * sizeof(float2);
    if (K.staged) {
#pragma unroll 4
        for (int i = tid; i < N; i += AL_T) {
            const LpdAlignPre q = lpd_align_pre(pa[3 * i], pa[3 * i + 1], pa[3 * i + 2], sa, K.z0, K.inv_zcell, L);
            sp[i] = q.ok ? make_float2(q.px, q.py) : make_float2(NAN, NAN);
            sl[i] = (unsigned char)q.iz;
        }
    }
    uint4* Am = Aw[wave];
    uint32_t* aw = (uint32_t*)Am;
    unsigned long long bestkey = 0ull;
    const int iters = (h1 - h0 + AL_WAVES - 1) / AL_WAVES;
    for (int it = 0; it < iters; ++it) {
        const int h = h0 + it * AL_WAVES + wave;
        const bool active = h < h1;      // uniform over the wave
        if (active)
            for (int i = lane; i < L * AL_G; i += 64) Am[i] = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        if (active) {
            const int ri = lpd_align_rot_index(f0, h, K.R);
            const float c = rot[2 * ri], s = rot[2 * ri + 1];
            if (K.staged) {      // written before the first of the two barriers above
#pragma unroll 4
                for (int i = lane; i < N; i += 64) {
                    const float2 q = sp[i];
                    const int iz = sl[i];
                    int ix, iy;
                    if (lpd_align_plan_a(q.x, q.y, c, s, has_t0, t0x, t0y, K.inv_cell, &ix, &iy))
                        atomicOr(&aw[((iz * AL_G + iy) << 2) + (ix >> 5)], 1u << (ix & 31));
                }
            } else {
#pragma unroll 4
                for (int i = lane; i < N; i += 64) {
                    const LpdAlignCell q = lpd_align_cell_a(pa[3 * i], pa[3 * i + 1], pa[3 * i + 2], sa, c, s, has_t0, t0x, t0y, K.inv_cell, K.z0,
                                                            K.inv_zcell, L);
                    if (q.valid) atomicOr(&aw[((q.iz * AL_G + q.iy) << 2) + (q.ix >> 5)], 1u << (q.ix & 31));
                }
            }
        }
        __syncthreads();
        if (!active) continue;
        // occupied cells of A under h, and which (layer, half) blocks hold any
        int nA = 0;
        unsigned blocks = 0u;
        for (int blk = 0; blk < 2 * L; ++blk) {
            const uint4 a = Am[(blk >> 1) * AL_G + (blk & 1) * 64 + lane];
            nA += __popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w);
            if (__ballot((a.x | a.y | a.z | a.w) != 0u)) blocks |= 1u << blk;
        }
        nA = al_wave_sum(nA);
        int ymax = 0;
        for (int dxi = 0; dxi <= twoS; ++dxi) {
            int acc[NDY];
#pragma unroll
            for (int j = 0; j < NDY; ++j) acc[j] = 0;
            for (int blk = 0; blk < 2 * L; ++blk) {
                if (!((blocks >> blk) & 1u)) continue;
                const int l = blk >> 1, row = (blk & 1) * 64 + lane;
                const uint4 a4 = Am[l * AL_G + row];
                const uint32_t a[4] = {a4.x, a4.y, a4.z, a4.w};
                uint32_t sh[4];
                lpd_align_shift128(a, dxi - S, sh);
                // row + dy + AL_PAD at [dy + S].  NDY >= 2S + 1 reads with no branch between them: behind a uniform guard per dy the
                // compiler made every read wait for the one before.  The reads behind 2S stay inside the layer's
                // AL_BROWS rows, and their sums are not looked at.
                const uint4* bp = Bp + l * AL_BROWS + row + AL_PAD - S;
#pragma unroll
                for (int dyi = 0; dyi < NDY; ++dyi) {
                    const uint4 b4 = bp[dyi];
                    const uint32_t b[4] = {b4.x, b4.y, b4.z, b4.w};
                    acc[dyi] += lpd_align_row_score(sh, b);
                }
            }
            // two sums to a word: a lane's sum is at most 1024 and the wave's at most N <= 16384, so the low half never carries
#pragma unroll
            for (int j = 0; 2 * j < NDY; ++j) {
                int v = acc[2 * j];
                if (2 * j + 1 < NDY) v |= acc[2 * j + 1] << 16;
                v = al_wave_sum(v);
                const int s0 = v & 0xFFFF, s1 = (int)((unsigned)v >> 16);
                const unsigned long long k0 = 2 * j <= twoS ? lpd_align_key(s0, h, 2 * j, dxi, nA) : 0ull;
                const unsigned long long k1 = 2 * j + 1 <= twoS ? lpd_align_key(s1, h, 2 * j + 1, dxi, nA) : 0ull;
                const unsigned long long k = k0 > k1 ? k0 : k1;
                bestkey = k > bestkey ? k : bestkey;
                const int m0 = 2 * j <= twoS ? s0 : 0, m1 = 2 * j + 1 <= twoS ? s1 : 0;
                ymax = max(ymax, max(m0, m1));
            }
        }
        if (yaw_scores && lane == 0) yaw_scores[(size_t)p * K.H + h] = ymax;
    }
    if (lane == 0) wkey[wave] = bestkey;      // 0 for a wave without a hypothesis: below every key of a candidate
    __syncthreads();
    if (tid != 0) return;
    unsigned long long key = wkey[0];
    for (int w = 1; w < AL_WAVES; ++w) key = wkey[w] > key ? wkey[w] : key;
    if (K.G == 1) {
        lpd_align_unkey(key, S, nB_s, best + 8 * (size_t)p);
    } else {
        ws[(size_t)p * K.G + g] = AlSlot{key, nB_s, 0};
    }
}

__global__ __launch_bounds__(AL_T) void align_finish_kernel(const int32_t* __restrict__ pairs, AlK K, const AlSlot* __restrict__ ws,
                                                            int32_t* __restrict__ best)
{
    const int p = blockIdx.x * AL_T + threadIdx.x;
    if (p >= K.P) return;
    int ra, rb;
    if (!al_pair_ok(pairs, p, K.TA, K.TB, &ra, &rb)) {
        al_write_missing(best + 8 * (size_t)p);
        return;
    }
    const AlSlot* s = ws + (size_t)p * K.G;
    unsigned long long key = s[0].key;
    for (int g = 1; g < K.G; ++g) key = s[g].key > key ? s[g].key : key;
    lpd_align_unkey(key, K.S, s[0].nB, best + 8 * (size_t)p);
}

inline bool al_dims_ok(int P, int H) { return P >= 1 && P <= LPD_ALIGN_MAX_PAIRS && H >= 1 && H <= LPD_ALIGN_MAX_H; }

}  // namespace

extern "C" long long lpd_align_workspace_bytes(int P, int H)
{
    if (!al_dims_ok(P, H)) return 0;
    int G, hs;
    al_split(P, H, &G, &hs);
    return G > 1 ? (long long)P * G * (long long)sizeof(AlSlot) : 0;
}

extern "C" int lpd_align_pairs(const float* A, int TA, const float* scaleA, const float* B, int TB, const float* scaleB, int N,
                               const int32_t* pairs, int P, const float* rot, int R, const int32_t* first, int H, const float* t0,
                               float inv_cell, int S, float z0, float inv_zcell, int layers, int32_t* best, int32_t* yaw_scores, void* ws,
                               void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(A && B && pairs && rot && best, "lpd_align_pairs: null pointer");
    LPD_CHECK_ARG(TA >= 1 && TB >= 1 && N >= 1 && N <= LPD_ALIGN_MAX_POINTS, "lpd_align_pairs: bad dims TA=%d TB=%d N=%d (>= 1, N <= %d)", TA, TB, N,
                  LPD_ALIGN_MAX_POINTS);
    LPD_CHECK_ARG(P >= 1 && P <= LPD_ALIGN_MAX_PAIRS, "lpd_align_pairs: P=%d outside 1 .. 2^20", P);
    LPD_CHECK_ARG(H >= 1 && H <= R && R <= LPD_ALIGN_MAX_R && H <= LPD_ALIGN_MAX_H, "lpd_align_pairs: 1 <= H=%d <= R=%d <= %d and H <= %d required", H,
                  R, LPD_ALIGN_MAX_R, LPD_ALIGN_MAX_H);
    LPD_CHECK_ARG(S >= 0 && S <= LPD_ALIGN_MAX_S, "lpd_align_pairs: S=%d outside 0 .. %d", S, LPD_ALIGN_MAX_S);
    LPD_CHECK_ARG(layers >= 1 && layers <= LPD_ALIGN_MAX_LAYERS, "lpd_align_pairs: layers=%d outside 1 .. %d", layers, LPD_ALIGN_MAX_LAYERS);
    LPD_CHECK_ARG(lpd_align_finite(inv_cell) && inv_cell > 0.0f && lpd_align_finite(inv_zcell) && inv_zcell > 0.0f && lpd_align_finite(z0),
                  "lpd_align_pairs: inv_cell=%g inv_zcell=%g (finite, > 0) z0=%g (finite)", (double)inv_cell, (double)inv_zcell, (double)z0);
    AlK K;
    K.TA = TA; K.TB = TB; K.N = N; K.P = P; K.R = R; K.H = H; K.S = S; K.layers = layers;
    K.inv_cell = inv_cell; K.z0 = z0; K.inv_zcell = inv_zcell;
    al_split(P, H, &K.G, &K.hs);
    K.staged = N <= AL_STAGE_N;
    const int dyn = K.staged ? N * (int)sizeof(float2) + ((N + 15) & ~15) : 0;
    LPD_CHECK_ARG(K.G == 1 || (ws && ((uintptr_t)ws & 15) == 0), "lpd_align_pairs: the workspace (lpd_align_workspace_bytes, 16-byte aligned) is missing");
    // 43 KiB of static LDS + up to 36 KiB of dynamic LDS: more than the 64 KiB a kernel gets without asking, inside gfx950's 160 KiB a
    // CU.  The attribute belongs to (kernel instance, device), so it is set with every launch that stages; its failure is reported.
#define AL_LAUNCH(NDY_)                                                                                                                         \
    do {                                                                                                                                        \
        if (dyn) {                                                                                                                              \
            const hipError_t e_ = hipFuncSetAttribute((const void*)align_kernel<NDY_>, hipFuncAttributeMaxDynamicSharedMemorySize,              \
                                                      AL_STAGE_N * 9);                                                                          \
            if (e_ != hipSuccess) {                                                                                                             \
                lpd_set_error("lpd_align_pairs: %d bytes of dynamic LDS refused: %s", AL_STAGE_N * 9, hipGetErrorString(e_));                   \
                return LPD_ERR_LAUNCH;                                                                                                          \
            }                                                                                                                                   \
        }                                                                                                                                       \
        hipLaunchKernelGGL(align_kernel<NDY_>, dim3((unsigned)((long long)P * K.G)), dim3(AL_T), dyn, stream, A, scaleA, B, scaleB, pairs, rot, \
                           first, t0, K, best, yaw_scores, (AlSlot*)ws);                                                                        \
    } while (0)
    if (S == 0) AL_LAUNCH(1);
    else if (S == 1) AL_LAUNCH(3);
    else if (S <= 4) AL_LAUNCH(9);
    else if (S <= 8) AL_LAUNCH(17);
    else AL_LAUNCH(33);
#undef AL_LAUNCH
    if (K.G > 1)
        hipLaunchKernelGGL(align_finish_kernel, dim3((P + AL_T - 1) / AL_T), dim3(AL_T), 0, stream, pairs, K, (const AlSlot*)ws, best);
    LPD_CHECK_LAUNCH("lpd_align_pairs");
    return LPD_OK;
}
