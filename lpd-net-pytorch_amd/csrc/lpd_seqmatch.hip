// lpd_seqmatch.hip -- lpd_seq_match: sequence scoring of retrieved place candidates along the drive (the definition is in
// include/lpd_hip.h, every detail in lpd_seq_math.h).
//
// All hypotheses (velocity, shift) of a candidate (query i, centre row j) read from ONE block of distances: query rows i-h .. i+h (at
// most 31) against database rows j-15 .. j+15 (31).  The block is therefore computed once per candidate as a single 32 x 32 tile of
// the exact f32-input MFMA over the channels, quantised to integers in LDS, and every hypothesis is then 2h+1 integer reads of LDS:
// 62 descriptor rows are fetched per candidate instead of V (2S+1) (2h+1) gathered ones.
//
// Tiling.  Workgroup = one query = 4 waves.
//   * The query's band is the MFMA's B operand and lives in registers for the whole workgroup (lane (c, hh): channels 2 s + hh of
//     query row i - h + c, zeros for c > 2h and for rows outside the table -- 128 VGPRs at dim 256), as recall_pairs_kernel holds its
//     queries; every wave holds a copy, read from one k-major staging of the band in LDS that the four waves fetch between them.
//   * Wave w takes the candidates r = w, w + 4, ...  It stages its candidate's database band k-major in its OWN quarter of the LDS
//     ([channel][row]: the operand fetch of an MFMA step is one conflict-free ds_read_b32 per lane), at most 64 channels at a time
//     (two parts at dim 64 and 128, four at dim 256): 8 KiB a wave, 34 KiB a workgroup, and 8 sixteen-byte loads a lane in flight
//     beside the 128 registers of the operand -- a part of 128 channels spilled.  Two workgroups share a CU (256 VGPRs each): one
//     fetches while the other computes.
//   * After the chain the wave quantises its 16 accumulators a lane into the [32][32] block (row stride 33: the 32 lanes of a half-wave
//     write 32 banks) in the same LDS, lanes take the hypotheses e = lane, lane + 64, ..., and the wave reduces (sum, n, e) by
//     lpd_seq_better through __shfl_xor: a total order, so the butterfly leaves the winner in every lane.
//   * After the last candidate wave 0 ranks the K <= 64 results: lane r counts the candidates that come before it.  O(K) reads, no sort.
// The waves' LDS areas are private, but what one lane writes another lane of the wave reads, and the block lies over the staged band:
// the phases are separated by __syncthreads() in uniform control flow (every wave runs every round; a wave without a candidate does
// nothing between the barriers).  No atomics.  Rows outside a table are never read: zeros go to the MFMA and the block says -1.
#include "lpd_common.h"
#include "lpd_seq_math.h"

namespace {

constexpr int SQ_THREADS = 256;
constexpr int SQ_WAVES = 4;
constexpr int SQ_BS = LPD_SEQ_TILE + 1;                 // row stride of the block in LDS
constexpr int SQ_BLK = LPD_SEQ_TILE * SQ_BS;            // ints of a block in LDS

__global__ void seq_rownorm_kernel(const float* __restrict__ X, int ld, int n, int dim, float* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int c = 0; c < dim; ++c) s = fmaf(X[(size_t)i * ld + c], X[(size_t)i * ld + c], s);
    out[i] = s;
}

struct SeqArgs {
    const float* Q; int ldq, nq;
    const float* D; int ldd, nd;
    const float* qn; const float* dn;      // squared norms of every row of Q / D
    const int32_t* q_off; int SQ;
    const int32_t* d_off; int SD;
    const int32_t* cand; int K;
    const int32_t* steps; int V, h, S, min_terms;
    int32_t* best; int32_t* order; int32_t* block;
};

// channels of a 32-row band that a wave stages at a time: half the channels, and at most 64 (16 bytes x 8 loads a lane in flight)
template <int KP>
constexpr int seq_part() { return KP < 64 ? KP : 64; }
// floats of a wave's LDS area: one part of the band, and not less than a block
template <int KP>
constexpr int seq_wave_area() { return seq_part<KP>() * LPD_SEQ_TILE > SQ_BLK ? seq_part<KP>() * LPD_SEQ_TILE : SQ_BLK; }

// KP = channel pairs held per lane: dim = 2 KP (64, 128 or 256)
template <int KP>
__global__ __launch_bounds__(SQ_THREADS, 2) void seq_match_kernel(SeqArgs a)
{
    constexpr int DIMH = seq_part<KP>();     // channels of a part
    constexpr int NP = 2 * KP / DIMH;        // parts: 2 at dim 64 and 128, 4 at dim 256
    constexpr int KH = DIMH / 2;             // MFMA steps of a part
    constexpr int NE = DIMH / 8;             // 16-byte loads a lane makes for a part: 32 rows x DIMH / 4 quads over 64 lanes
    constexpr int WAREA = seq_wave_area<KP>();
    extern __shared__ __attribute__((aligned(16))) float sq_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 31, hh = lane >> 5;
    float* dt = sq_lds + wave * WAREA;                                        // [DIMH][32] this wave's staged part of the band, k-major
    int32_t* blk = reinterpret_cast<int32_t*>(dt);                            // [32][SQ_BS] this wave's block (after the chain)
    float* dnl = sq_lds + SQ_WAVES * WAREA + wave * LPD_SEQ_TILE;             // [32] squared norms of this wave's band
    int32_t* res = reinterpret_cast<int32_t*>(sq_lds + SQ_WAVES * WAREA + SQ_WAVES * LPD_SEQ_TILE);      // [LPD_SEQ_KMAX][4] the results

    const int i = blockIdx.x;
    const int h = a.h, L = 2 * h + 1;
    int qlo, qhi;
    {
        const int m = lpd_seq_run(a.q_off, a.SQ, i);
        qlo = a.q_off[m];
        qhi = a.q_off[m + 1];
    }

    // the query band as the B operand: lane (c, hh) holds channels 2 s + hh of query row i - h + c
    const int qa = i - h + c;
    const bool qok = c < L && qa >= 0 && qa < a.nq;
    // The four waves fetch the band once between them (16-byte loads; thread (row, g) moves the quads g + 8 e of its row), lay it
    // k-major over the waves' areas, and every wave reads its copy of the operand from there: a lane's own loads would be 4 bytes
    // from each of 32 rows an instruction, four times over.
    float qreg[KP];
    {
        constexpr int NQ = KP / 16;
        const int row = tid & 31, g = tid >> 5;
        const int qr = i - h + row;
        const bool rok = row < L && qr >= 0 && qr < a.nq;
        const float* qrow = a.Q + (size_t)(rok ? qr : 0) * a.ldq;
        float4 pre[NQ];
#pragma unroll
        for (int e = 0; e < NQ; ++e) pre[e] = rok ? *reinterpret_cast<const float4*>(qrow + 4 * (g + 8 * e)) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int e = 0; e < NQ; ++e) {
            const int kk = 4 * (g + 8 * e);
            sq_lds[(kk + 0) * LPD_SEQ_TILE + row] = pre[e].x;
            sq_lds[(kk + 1) * LPD_SEQ_TILE + row] = pre[e].y;
            sq_lds[(kk + 2) * LPD_SEQ_TILE + row] = pre[e].z;
            sq_lds[(kk + 3) * LPD_SEQ_TILE + row] = pre[e].w;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < KP; ++s) qreg[s] = sq_lds[(2 * s + hh) * LPD_SEQ_TILE + c];
        // (the first barrier of the first round stands between these reads and the staging of the database bands)
    }
    static_assert(2 * KP * LPD_SEQ_TILE <= SQ_WAVES * WAREA, "the query band is staged over the waves' areas");
    const float qn = qok ? a.qn[qa] : 0.f;

    const int W = 2 * a.S + 1, E = a.V * W;
    const int rounds = (a.K + SQ_WAVES - 1) / SQ_WAVES;
    for (int rd = 0; rd < rounds; ++rd) {
        const int r = rd * SQ_WAVES + wave;
        const bool active = r < a.K;                                          // (uniform in the wave)
        const int j = active ? a.cand[(size_t)i * a.K + r] : -1;
        const bool live = active && j >= 0 && j < a.nd;

        f32x16 acc;
#pragma unroll
        for (int x = 0; x < 16; ++x) acc[x] = 0.f;
        // staging: lane (c = row of the band, hh) moves the quads hh + 2 e of its row
        const int brow = j - LPD_SEQ_BAND + c;
        const bool bok = live && c < LPD_SEQ_TILE - 1 && brow >= 0 && brow < a.nd;
        const float* drow = a.D + (size_t)(bok ? brow : 0) * a.ldd;
#pragma unroll
        for (int half = 0; half < NP; ++half) {
            float4 pre[NE];
#pragma unroll
            for (int e = 0; e < NE; ++e)
                pre[e] = bok ? *reinterpret_cast<const float4*>(drow + half * DIMH + 4 * (hh + 2 * e)) : make_float4(0.f, 0.f, 0.f, 0.f);
            float pre_n = 0.f;
            if (half == 0 && hh == 0) pre_n = bok ? a.dn[brow] : 0.f;
            __syncthreads();                                                  // the last readers of this area are done
            if (live) {
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const int kk = 4 * (hh + 2 * e);
                    dt[(kk + 0) * LPD_SEQ_TILE + c] = pre[e].x;
                    dt[(kk + 1) * LPD_SEQ_TILE + c] = pre[e].y;
                    dt[(kk + 2) * LPD_SEQ_TILE + c] = pre[e].z;
                    dt[(kk + 3) * LPD_SEQ_TILE + c] = pre[e].w;
                }
                if (half == 0 && hh == 0) dnl[c] = pre_n;
            }
            __syncthreads();
            if (live) {
                const float* ap = dt + hh * LPD_SEQ_TILE + c;
#pragma unroll
                for (int s = 0; s < KH; ++s)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s * LPD_SEQ_TILE], qreg[half * KH + s], acc, 0, 0, 0);
            }
        }
        __syncthreads();                                                      // the chain has read the band: the block may lie over it
        if (active) {
            // lane (c, hh) holds query row c of the band against database rows (x & 3) + 8 (x >> 2) + 4 hh
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int row = (x & 3) + 8 * (x >> 2) + 4 * hh;
                const int b = j - LPD_SEQ_BAND + row;
                const bool ok = live && qok && row < LPD_SEQ_TILE - 1 && b >= 0 && b < a.nd;
                blk[c * SQ_BS + row] = ok ? lpd_seq_d2q(qn, dnl[row], acc[x]) : -1;
            }
        }
        __syncthreads();
        if (active) {
            int32_t bs = 0, bn = 0;
            int be = -1;
            if (live) {
                int dlo, dhi;
                {
                    const int m = lpd_seq_run(a.d_off, a.SD, j);
                    dlo = max(a.d_off[m], 0);
                    dhi = min(a.d_off[m + 1], a.nd);
                }
                for (int e = lane; e < E; e += 64) {
                    const int v = lpd_seq_hyp_v(e, a.S), s = lpd_seq_hyp_s(e, a.S);
                    if (!lpd_seq_centre_ok(j, s, dlo, dhi)) continue;
                    const LpdSeqSum t = lpd_seq_hypothesis(blk, SQ_BS, a.steps + (size_t)v * L, h, s, i, qlo, qhi, j, dlo, dhi);
                    if (t.n >= a.min_terms && lpd_seq_better(t.sum, t.n, e, bs, bn, be)) { bs = t.sum; bn = t.n; be = e; }
                }
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) {
                    const int32_t os = __shfl_xor(bs, m, 64), on = __shfl_xor(bn, m, 64);
                    const int oe = __shfl_xor(be, m, 64);
                    if (lpd_seq_better(os, on, oe, bs, bn, be)) { bs = os; bn = on; be = oe; }
                }
            }
            if (lane == 0) {
                const int32_t o0 = be, o1 = be < 0 ? 0 : bs, o2 = be < 0 ? 0 : bn, o3 = be < 0 ? -1 : j + lpd_seq_hyp_s(be, a.S);
                int32_t* o = a.best + ((size_t)i * a.K + r) * 4;
                o[0] = o0; o[1] = o1; o[2] = o2; o[3] = o3;
                res[4 * r + 0] = o0; res[4 * r + 1] = o1; res[4 * r + 2] = o2; res[4 * r + 3] = o3;
            }
            if (a.block) {
                int32_t* o = a.block + ((size_t)i * a.K + r) * (LPD_SEQ_TILE * LPD_SEQ_TILE);
                for (int x = lane; x < LPD_SEQ_TILE * LPD_SEQ_TILE; x += 64) o[x] = blk[(x >> 5) * SQ_BS + (x & 31)];
            }
        }
    }
    __syncthreads();
    // the order of the candidates: lane r counts those that come before it
    if (tid < a.K) {
        const int r = tid;
        const int32_t me = res[4 * r], ms = res[4 * r + 1], mn = res[4 * r + 2];
        int before = 0;
        for (int o = 0; o < a.K; ++o) {
            const int32_t oe = res[4 * o], os = res[4 * o + 1], on = res[4 * o + 2];
            const bool first = me >= 0 ? lpd_seq_better(os, on, oe < 0 ? -1 : o, ms, mn, r) : (oe >= 0 || o < r);
            before += first ? 1 : 0;
        }
        a.order[(size_t)i * a.K + before] = r;
    }
}

template <int KP>
int launch_seq(const SeqArgs& a, hipStream_t stream)
{
    const size_t lds = ((size_t)SQ_WAVES * seq_wave_area<KP>() + SQ_WAVES * LPD_SEQ_TILE + LPD_SEQ_KMAX * 4) * sizeof(float);
    (void)hipFuncSetAttribute((const void*)seq_match_kernel<KP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(seq_match_kernel<KP>, dim3(a.nq), dim3(SQ_THREADS), lds, stream, a);
    LPD_CHECK_LAUNCH("lpd_seq_match");
    return LPD_OK;
}

}  // namespace

extern "C" int lpd_seq_match(const float* Q, int ldq, int nq, const int32_t* q_off, int SQ, const float* D, int ldd, int nd, const int32_t* d_off,
                             int SD, int dim, const int32_t* cand, int K, const int32_t* steps, int V, int h, int S, int min_terms, int32_t* best,
                             int32_t* order, int32_t* block, float* ws, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(Q && D && q_off && d_off && cand && steps && best && order && ws, "lpd_seq_match: null pointer");
    LPD_CHECK_ARG((dim == 64 || dim == 128 || dim == 256) && ldq >= dim && ldd >= dim && ldq % 4 == 0 && ldd % 4 == 0 &&
                  (((uintptr_t)Q | (uintptr_t)D) & 15) == 0,
                  "lpd_seq_match: dim=%d (64, 128 or 256), ldq=%d, ldd=%d (multiples of 4, 16-byte aligned rows)", dim, ldq, ldd);
    LPD_CHECK_ARG(nq > 0 && nd > 0 && SQ > 0 && SD > 0, "lpd_seq_match: bad sizes nq=%d nd=%d SQ=%d SD=%d", nq, nd, SQ, SD);
    LPD_CHECK_ARG(K > 0 && K <= LPD_SEQ_KMAX, "lpd_seq_match: K=%d (1..%d)", K, LPD_SEQ_KMAX);
    LPD_CHECK_ARG(h >= 1 && h <= LPD_SEQ_BAND && S >= 0 && S <= LPD_SEQ_BAND, "lpd_seq_match: h=%d (1..%d), S=%d (0..%d)", h, LPD_SEQ_BAND, S, LPD_SEQ_BAND);
    LPD_CHECK_ARG(V > 0 && V <= LPD_SEQ_MAX_HYP && V * (2 * S + 1) <= LPD_SEQ_MAX_HYP, "lpd_seq_match: V=%d, S=%d: V (2S+1) must lie in 1..%d", V, S,
                  LPD_SEQ_MAX_HYP);
    LPD_CHECK_ARG(min_terms >= 1 && min_terms <= 2 * h + 1, "lpd_seq_match: min_terms=%d (1..%d)", min_terms, 2 * h + 1);
    float* qn = ws;            // [nq]
    float* dn = ws + nq;       // [nd]
    hipLaunchKernelGGL(seq_rownorm_kernel, dim3((nq + 255) / 256), dim3(256), 0, stream, Q, ldq, nq, dim, qn);
    hipLaunchKernelGGL(seq_rownorm_kernel, dim3((nd + 255) / 256), dim3(256), 0, stream, D, ldd, nd, dim, dn);
    LPD_CHECK_LAUNCH("lpd_seq_match (norms)");
    SeqArgs a;
    a.Q = Q; a.ldq = ldq; a.nq = nq; a.D = D; a.ldd = ldd; a.nd = nd; a.qn = qn; a.dn = dn;
    a.q_off = q_off; a.SQ = SQ; a.d_off = d_off; a.SD = SD; a.cand = cand; a.K = K;
    a.steps = steps; a.V = V; a.h = h; a.S = S; a.min_terms = min_terms;
    a.best = best; a.order = order; a.block = block;
    if (dim == 64) return launch_seq<32>(a, stream);
    if (dim == 128) return launch_seq<64>(a, stream);
    return launch_seq<128>(a, stream);
}
