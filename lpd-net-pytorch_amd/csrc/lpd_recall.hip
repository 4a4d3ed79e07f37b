// lpd_recall.hip -- the whole recall evaluation of evaluate.py:33-93 (every (database run m, query run n) pair of
// evaluate_model, each scored as in get_recall, evaluate.py:162-206) in ONE launch over descriptor tables that stay on the device.
//
// Per (pair, query): the k nearest database rows of run m by squared L2 distance, ties -> lower index, with the arithmetic of
// lpd_retrieval_topk (|q|^2 + |d|^2 - 2 q.d clamped at 0; norms by an fmaf chain in channel order; q.d on the exact f32-input MFMA,
// which is the k-ordered fmaf chain bit for bit, so the distances -- and the rankings -- are those of lpd_retrieval_topk), then the
// first rank that holds a true neighbour, the one-percent flag and the rank-0 similarity.  Nothing of size n_q x n_db is stored.
//
// Tiling.  Workgroup = 4 waves = 128 queries of run n (32 per wave); it streams run m's rows through LDS 32 at a time:
//   * the wave's 32 queries are the MFMA's B operand and live in registers for the whole launch (lane (c, h): query c, channels
//     2 s + h, s < DIMP / 2 -- 128 VGPRs at dim 256); the database tile is the A operand, staged k-major in LDS ([channel][row]: the
//     operand fetch of step s is one conflict-free ds_read_b32 per lane), shared by the four waves;
//   * one v_mfma_f32_32x32x2_f32 chain of DIMP / 2 steps per tile gives the 32 x 32 dot products: lane (c, h) holds query c against
//     rows (r & 3) + 8 (r >> 2) + 4 h, r < 16.  The upper half-wave hands its 16 distances to lane c (one swizzle each), which then
//     meets its query's 32 candidates in ascending row order;
//   * lane c keeps its query's running top-k as a sorted list in LDS ([slot][query]: conflict-free).  A candidate is inserted only if
//     it is strictly closer than the current k-th entry (the threshold, a register; the passing ones wait in LDS for one rolled insert
//     loop); candidates arrive in ascending index, so the
//     strict test and the walk that stops at the first entry <= it are exactly the (distance, index) order.  At k = 25 nearly all
//     candidates fail the threshold after the first tiles: the insert branch is skipped wave-wide;
//   * after the last tile the same lane walks its truth list (CSR, built once per evaluation) against the ranks, recomputes the
//     rank-0 dot product by the fmaf chain, and the block adds its per-pair histogram to the caller's counts (LDS first, then one
//     atomic per non-empty bin).
// Two workgroups per CU at k = 25 and dim 256 (LDS: 32 KiB tile + 25 KiB lists + 16 KiB candidates = 73 KiB each; 230 VGPRs, no spills):
// one stages a tile while the other computes.
#include "lpd_common.h"

namespace {

constexpr int RP_THREADS = 256;
constexpr int RP_QT = 128;         // queries per workgroup (32 per wave)
constexpr int RP_DT = 32;          // database rows per tile
constexpr int RP_KMAX = LPD_RECALL_KMAX;

__global__ void recall_rownorm_kernel(const float* __restrict__ X, int ld, int n, int dim, float* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int c = 0; c < dim; ++c) s = fmaf(X[(size_t)i * ld + c], X[(size_t)i * ld + c], s);
    out[i] = s;
}

struct RecallArgs {
    const float* Q; int ldq;
    const float* D; int ldd;
    int dim;
    const float* qn; const float* dn;      // squared norms of every row of Q / D
    const int32_t* q_off; const int32_t* d_off;
    const int32_t* pairs; const int32_t* out_off;
    int npairs, max_qtiles, rd, k;
    const int32_t* truth_off; const int32_t* truth_idx;
    int32_t* first; uint8_t* one_pct; float* top1_sim; int32_t* topk_idx;
    int32_t* hist; int32_t* n_eval; int32_t* n_onepct;
};

// KP = channel pairs held per lane: dim = 2 KP (64, 128 or 256; rows 16-byte aligned -- the caller pads other sizes with zero channels,
// which add nothing to the fmaf chains)
template <int KP>
__global__ __launch_bounds__(RP_THREADS, 2) void recall_pairs_kernel(RecallArgs a)
{
    constexpr int DIMP = 2 * KP;
    extern __shared__ __attribute__((aligned(16))) float rp_lds[];
    float* dt = rp_lds;                                       // [DIMP][RP_DT] database tile, k-major
    float* dnl = dt + DIMP * RP_DT;                           // [RP_DT] its squared norms
    float* ld = dnl + RP_DT;                                  // [k][RP_QT] sorted distances of every query's top-k
    int* li = reinterpret_cast<int*>(ld + a.k * RP_QT);       // [k][RP_QT] their row numbers in run m
    float* cd = reinterpret_cast<float*>(li + a.k * RP_QT);   // [RP_DT][RP_QT] candidates of the current tile that pass the threshold
    int* sh = reinterpret_cast<int*>(cd + RP_DT * RP_QT);     // [k + 1] histogram, n_eval, one-percent count

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 31, h = lane >> 5;
    int bx, p;
    {
        const int lin = blockIdx.x + a.max_qtiles * blockIdx.y;     // the query tiles of one pair on one XCD (they stream the same run)
        const int v = lpd_xcd_remap(lin, a.max_qtiles * a.npairs);
        bx = v % a.max_qtiles;
        p = v / a.max_qtiles;
    }
    const int m = a.pairs[2 * p], n = a.pairs[2 * p + 1];
    const int qbase = a.q_off[n], nq = a.q_off[n + 1] - qbase;
    const int dbase = a.d_off[m], ndb = a.d_off[m + 1] - dbase;
    const int q0 = bx * RP_QT;
    if (q0 >= nq || ndb <= 0) return;                         // (uniform) this pair has fewer query tiles
    const int kp = min(a.k, ndb);
    for (int i = tid; i < a.k + 3; i += RP_THREADS) sh[i] = 0;
    for (int i = tid; i < kp * RP_QT; i += RP_THREADS) { ld[i] = INFINITY; li[i] = 0; }    // (rows stay in range whatever the data)

    // the wave's queries as the B operand: lane (c, h) holds channels 2 s + h of query q0 + 32 wave + c
    const int ql = q0 + wave * 32 + c;                        // query of this lane, inside run n
    const bool qvalid = ql < nq;
    float qreg[KP];
    {
        const float* qrow = a.Q + (size_t)(qbase + (qvalid ? ql : 0)) * a.ldq;
#pragma unroll
        for (int s = 0; s < KP; ++s) qreg[s] = qvalid ? qrow[2 * s + h] : 0.f;
    }
    const float qn = qvalid ? a.qn[qbase + ql] : 0.f;
    const int me = wave * 32 + c;                             // list column of this lane's query
    // only the lower half-wave owns lists; -inf: nothing passes
    float thr = (h == 0 && qvalid) ? INFINITY : -INFINITY;
    int cnt = 0;

    // tile staging: thread (r = tid & 31, quad kq = tid >> 5 + 8 e) moves 4 channels of row r
    constexpr int NE = DIMP / 4 / 8;
    const int sr = tid & 31, skq = tid >> 5;
    float4 pre[NE];
    float pre_n = 0.f;
    auto fetch = [&](int d0) {
        const int j = d0 + sr;
        const bool ok = j < ndb;
        const float* row = a.D + (size_t)(dbase + (ok ? j : 0)) * a.ldd;
#pragma unroll
        for (int e = 0; e < NE; ++e) pre[e] = ok ? *reinterpret_cast<const float4*>(row + 4 * (skq + 8 * e)) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid < RP_DT) pre_n = ok ? a.dn[dbase + j] : 0.f;
    };
    auto stage = [&]() {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int kk = 4 * (skq + 8 * e);
            dt[(kk + 0) * RP_DT + sr] = pre[e].x;
            dt[(kk + 1) * RP_DT + sr] = pre[e].y;
            dt[(kk + 2) * RP_DT + sr] = pre[e].z;
            dt[(kk + 3) * RP_DT + sr] = pre[e].w;
        }
        if (tid < RP_DT) dnl[tid] = pre_n;
    };

    fetch(0);
    stage();
    __syncthreads();
    for (int d0 = 0; d0 < ndb; d0 += RP_DT) {
        const bool more = d0 + RP_DT < ndb;
        if (more) fetch(d0 + RP_DT);                          // next tile in flight under this one's MFMA chain
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float* ap = dt + h * RP_DT + c;
#pragma unroll
        for (int s = 0; s < KP; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s * RP_DT], qreg[s], acc, 0, 0, 0);
        // distances of this lane's 16 rows (past the run: +inf, never inserted)
        float dv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            dv[r] = d0 + row < ndb ? fmaxf(qn + dnl[row] - 2.0f * acc[r], 0.0f) : INFINITY;
        }
        // the lower half-wave's candidate mask, bit = row in the tile (upper half's rows arrive by swizzle): ascending bits are
        // ascending rows.  Passing candidates go through LDS so that ONE rolled insert loop serves all 32.
        unsigned mask = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2);
            const float pv = __shfl_xor(dv[r], 32, 64);
            if (dv[r] < thr) { mask |= 1u << row; cd[row * RP_QT + me] = dv[r]; }
            if (pv < thr) { mask |= 1u << (row + 4); cd[(row + 4) * RP_QT + me] = pv; }
        }
        while (mask) {
            const int row = __builtin_ctz(mask);
            mask &= mask - 1;
            const float d = cd[row * RP_QT + me];
            if (!(d < thr)) continue;                        // (the threshold has moved since the mask was taken)
            const int j = d0 + row;
            int pos = cnt < kp ? cnt : kp - 1;
            while (pos > 0) {
                const float pd = ld[(pos - 1) * RP_QT + me];
                if (pd <= d) break;
                ld[pos * RP_QT + me] = pd;
                li[pos * RP_QT + me] = li[(pos - 1) * RP_QT + me];
                --pos;
            }
            ld[pos * RP_QT + me] = d;
            li[pos * RP_QT + me] = j;
            if (cnt < kp) ++cnt;
            if (cnt == kp) thr = ld[(kp - 1) * RP_QT + me];
        }
        __syncthreads();                                      // every wave is done with this tile
        if (more) {
            stage();
            __syncthreads();
        }
    }

    if (h == 0 && qvalid) {
        const int gq = qbase + ql;
        const int row_out = a.out_off[p] + ql;
        const long long tb = (long long)gq * a.rd + m;
        const int t0 = a.truth_off[tb], t1 = a.truth_off[tb + 1];
        int first = -1;
        if (t1 > t0) {
            first = a.k;
            for (int r = 0; r < kp && first == a.k; ++r) {
                const int j = li[r * RP_QT + me];
                for (int t = t0; t < t1; ++t)
                    if (a.truth_idx[t] == j) { first = r; break; }
            }
        }
        // one-percent recall: a true neighbour within the first max(round(n_db / 100), 1) ranks (Python's round: half to even)
        int t1p = ndb / 100;
        const int rem = ndb % 100;
        if (rem > 50 || (rem == 50 && (t1p & 1))) ++t1p;
        t1p = min(max(t1p, 1), kp);
        const bool one = first >= 0 && first < t1p;
        // similarity with the rank-0 row: the fmaf chain the MFMA computed
        const int j0 = li[me];
        const float* qrow = a.Q + (size_t)gq * a.ldq;
        const float* drow = a.D + (size_t)(dbase + j0) * a.ldd;
        float sim = 0.f;
        for (int ch = 0; ch < a.dim; ++ch) sim = fmaf(qrow[ch], drow[ch], sim);
        a.first[row_out] = first;
        a.one_pct[row_out] = one ? 1 : 0;
        a.top1_sim[row_out] = sim;
        if (a.topk_idx) {
            int32_t* o = a.topk_idx + (size_t)row_out * a.k;
            for (int r = 0; r < a.k; ++r) o[r] = r < kp ? li[r * RP_QT + me] : -1;
        }
        if (first >= 0) {
            atomicAdd(&sh[first], 1);
            atomicAdd(&sh[a.k + 1], 1);
            if (one) atomicAdd(&sh[a.k + 2], 1);
        }
    }
    __syncthreads();
    if (tid <= a.k + 2) {
        const int v = sh[tid];
        if (v) atomicAdd(tid <= a.k ? a.hist + (size_t)p * (a.k + 1) + tid : (tid == a.k + 1 ? a.n_eval + p : a.n_onepct + p), v);
    }
}

template <int KP>
int launch_recall(const RecallArgs& a, hipStream_t stream)
{
    const size_t lds = ((size_t)2 * KP * RP_DT + RP_DT + (size_t)2 * a.k * RP_QT + RP_DT * RP_QT + RP_KMAX + 3) * sizeof(float);
    (void)hipFuncSetAttribute((const void*)recall_pairs_kernel<KP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(recall_pairs_kernel<KP>, dim3(a.max_qtiles, a.npairs), dim3(RP_THREADS), lds, stream, a);
    LPD_CHECK_LAUNCH("lpd_recall_pairs");
    return LPD_OK;
}

}  // namespace

extern "C" int lpd_recall_pairs(const float* Q, int ldq, const float* D, int ldd, int dim, const int32_t* q_off, const int32_t* d_off, int rd,
                                int q_rows, int d_rows, const int32_t* pairs, const int32_t* out_off, int npairs, int max_qtiles,
                                const int32_t* truth_off, const int32_t* truth_idx, int k, int32_t* first, uint8_t* one_pct,
                                float* top1_sim, int32_t* topk_idx, int32_t* hist, int32_t* n_eval, int32_t* n_onepct, float* ws,
                                void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(Q && D && q_off && d_off && pairs && out_off && truth_off && truth_idx && first && one_pct && top1_sim && hist && n_eval &&
                  n_onepct && ws, "lpd_recall_pairs: null pointer");
    LPD_CHECK_ARG((dim == 64 || dim == 128 || dim == 256) && ldq >= dim && ldd >= dim && ldq % 4 == 0 && ldd % 4 == 0 &&
                  (((uintptr_t)Q | (uintptr_t)D) & 15) == 0,
                  "lpd_recall_pairs: dim=%d (64, 128 or 256), ldq=%d, ldd=%d (multiples of 4, 16-byte aligned rows)", dim, ldq, ldd);
    LPD_CHECK_ARG(k > 0 && k <= RP_KMAX, "lpd_recall_pairs: k=%d (1..%d)", k, RP_KMAX);
    LPD_CHECK_ARG(rd > 0 && q_rows > 0 && d_rows > 0 && npairs > 0 && max_qtiles > 0 && npairs <= 65535,
                  "lpd_recall_pairs: bad sizes rd=%d q_rows=%d d_rows=%d npairs=%d max_qtiles=%d", rd, q_rows, d_rows, npairs, max_qtiles);
    float* qn = ws;               // [q_rows]
    float* dn = ws + q_rows;      // [d_rows]
    hipLaunchKernelGGL(recall_rownorm_kernel, dim3((q_rows + 255) / 256), dim3(256), 0, stream, Q, ldq, q_rows, dim, qn);
    hipLaunchKernelGGL(recall_rownorm_kernel, dim3((d_rows + 255) / 256), dim3(256), 0, stream, D, ldd, d_rows, dim, dn);
    (void)hipMemsetAsync(hist, 0, sizeof(int32_t) * (size_t)npairs * (k + 1), stream);
    (void)hipMemsetAsync(n_eval, 0, sizeof(int32_t) * (size_t)npairs, stream);
    (void)hipMemsetAsync(n_onepct, 0, sizeof(int32_t) * (size_t)npairs, stream);
    LPD_CHECK_LAUNCH("lpd_recall_pairs (norms)");
    RecallArgs a;
    a.Q = Q; a.ldq = ldq; a.D = D; a.ldd = ldd; a.dim = dim; a.qn = qn; a.dn = dn;
    a.q_off = q_off; a.d_off = d_off; a.pairs = pairs; a.out_off = out_off;
    a.npairs = npairs; a.max_qtiles = max_qtiles; a.rd = rd; a.k = k;
    a.truth_off = truth_off; a.truth_idx = truth_idx;
    a.first = first; a.one_pct = one_pct; a.top1_sim = top1_sim; a.topk_idx = topk_idx;
    a.hist = hist; a.n_eval = n_eval; a.n_onepct = n_onepct;
    if (dim == 64) return launch_recall<32>(a, stream);
    if (dim == 128) return launch_recall<64>(a, stream);
    return launch_recall<128>(a, stream);
}
