// lpd_feat.hip -- local point-distribution features: the five handcrafted per-point columns behind xyz that the use_mFea trunks
// of LPD-Net take (reference lpdnet_model.py:183-186,215-224 reads them from an offline preprocessing step), computed on the device
// from each point's sorted kNN list.  Definition of the ten columns: include/lpd_hip.h; arithmetic: lpd_feat_math.h.
//
// One lane per point.  The lane walks its list ONCE, nearest first, accumulating the moments of d_j = x_{n_j} - x_i; the candidate
// neighbourhood sizes of the adaptive form are prefixes of that walk: after the k-th entry of a candidate size k the lane solves the
// 3x3 eigenproblem of the moments so far and keeps them when their eigenentropy is the smallest yet.  The candidate sizes arrive as a
// 64-bit mask (bit k-1 = "evaluate after k entries"; K <= 64), a kernel argument -- no device copy of the host array.
//
// Two forms of the neighbour read, same arithmetic, same bits:
//   LDS form  (N <= 4096)  the cloud's coordinates, 12 N bytes, are staged in LDS by each 512-thread block (48 KiB: three blocks per
//                          CU); the 3 K gathers of a lane are LDS reads.
//   L2 form   (larger N)   the gathers go to global memory; a cloud's coordinates (48 N bytes of distinct lines at most) stay in L2,
//                          and Z-ordered clouds (lpd_morton_sort) make the lists of neighbouring lanes hit the same lines.
// The index lists are the only sizeable traffic (4 K bytes per point).  A list is a contiguous row: with K % 4 == 0 and a 16-byte
// aligned base the lane reads it as int4 pieces (each 64-byte line of a row is consumed by one lane in consecutive iterations and is
// fetched once); other K take 4-byte loads.
#include "lpd_common.h"
#include "lpd_feat_math.h"

namespace {

constexpr int FEAT_LDS_MAX_N = 4096;      // 12 N bytes of LDS: 48 KiB
constexpr int FEAT_T_LDS = 512, FEAT_T_L2 = 256;

template <bool LDS>
__global__ __launch_bounds__(LDS ? FEAT_T_LDS : FEAT_T_L2) void local_features_kernel(
    const float* __restrict__ xyz, int ldx, const int32_t* __restrict__ idx, int N, int K, int kmax, unsigned long long evalmask,
    unsigned sel, int copy_xyz, float* __restrict__ out, int ldo, int32_t* __restrict__ kopt, int vec4)
{
    extern __shared__ __attribute__((aligned(16))) float cloud[];      // [N][3] (LDS form)
    constexpr int T = LDS ? FEAT_T_LDS : FEAT_T_L2;
    const int tiles = (N + T - 1) / T;
    const int b = blockIdx.x / tiles, i = (blockIdx.x % tiles) * T + (int)threadIdx.x;
    const float* xc = xyz + (size_t)b * N * ldx;
    if (LDS) {
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
    if (i >= N) return;
    float px, py, pz;
    if (LDS) { px = cloud[3 * i]; py = cloud[3 * i + 1]; pz = cloud[3 * i + 2]; }
    else { px = xc[(size_t)i * ldx]; py = xc[(size_t)i * ldx + 1]; pz = xc[(size_t)i * ldx + 2]; }
    const int32_t* row = idx + ((size_t)b * N + i) * K;

    LpdFeatMoments m, best;
    lpd_feat_init(m);
    best = m;
    float best_a = INFINITY;
    int best_k = 0;
    for (int j0 = 0; j0 < kmax; j0 += 4) {
        int4 q;
        if (vec4) q = *reinterpret_cast<const int4*>(row + j0);      // K % 4 == 0: j0 + 3 < K
        else {
            q.x = row[j0];
            q.y = j0 + 1 < kmax ? row[j0 + 1] : 0;
            q.z = j0 + 2 < kmax ? row[j0 + 2] : 0;
            q.w = j0 + 3 < kmax ? row[j0 + 3] : 0;
        }
        // "any list is legal": an index outside the cloud reads the cloud's last point instead of someone else's memory
        const unsigned last = (unsigned)(N - 1);
        const unsigned n0 = min((unsigned)q.x, last), n1 = min((unsigned)q.y, last), n2 = min((unsigned)q.z, last), n3 = min((unsigned)q.w, last);
        float cx[4], cy[4], cz[4];      // the four gathers are issued together; the accumulation below is in list order
        const unsigned nn[4] = {n0, n1, n2, n3};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (LDS) { cx[t] = cloud[3 * nn[t]]; cy[t] = cloud[3 * nn[t] + 1]; cz[t] = cloud[3 * nn[t] + 2]; }
            else { const float* pn = xc + (size_t)nn[t] * ldx; cx[t] = pn[0]; cy[t] = pn[1]; cz[t] = pn[2]; }
        }
#pragma unroll 1
        for (int t = 0; t < 4; ++t) {
            const int j = j0 + t;
            if (j >= kmax) break;
            const float nx = t == 0 ? cx[0] : t == 1 ? cx[1] : t == 2 ? cx[2] : cx[3];
            const float ny = t == 0 ? cy[0] : t == 1 ? cy[1] : t == 2 ? cy[2] : cy[3];
            const float nz = t == 0 ? cz[0] : t == 1 ? cz[1] : t == 2 ? cz[2] : cz[3];
            lpd_feat_add(m, nx - px, ny - py, nz - pz);
            if ((evalmask >> j) & 1ull) {      // a candidate size ends here (uniform: the mask is a kernel argument)
                const float a = lpd_feat_entropy(lpd_feat_eig(lpd_feat_cov(m, j + 1)));
                if (a < best_a) {              // strict: ties go to the smaller size
                    best_a = a;
                    best = m;
                    best_k = j + 1;
                }
            }
        }
    }
    float f[LPD_FEAT_COLUMNS];
    lpd_feat_columns(best, best_k, f);
    const size_t mrow = (size_t)b * N + i;
    float* o = out + mrow * ldo;
    int w = 0;
    if (copy_xyz) {
        o[0] = px;
        o[1] = py;
        o[2] = pz;
        w = 3;
    }
#pragma unroll
    for (int c = 0; c < LPD_FEAT_COLUMNS; ++c)
        if ((sel >> c) & 1u) o[w++] = f[c];
    if (kopt) kopt[mrow] = best_k;
}

}  // namespace

extern "C" int lpd_local_features(const float* xyz, int ldx, const int32_t* idx, int B, int N, int K, const int32_t* cand, int ncand,
                                  unsigned sel, int copy_xyz, float* out, int ldo, int32_t* kopt, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(xyz && idx && out, "lpd_local_features: null pointer");
    LPD_CHECK_ARG(B > 0 && N > 0 && ldx >= 3, "lpd_local_features: bad dims B=%d N=%d ldx=%d", B, N, ldx);
    LPD_CHECK_ARG(K >= 4 && K <= 64 && K <= N, "lpd_local_features: need 4 <= K <= 64 and K <= N (K=%d N=%d)", K, N);
    LPD_CHECK_ARG((long long)B * N < (1ll << 31), "lpd_local_features: B * N = %lld rows exceed 2^31", (long long)B * N);
    LPD_CHECK_ARG(copy_xyz == 0 || copy_xyz == 1, "lpd_local_features: copy_xyz=%d (0 or 1)", copy_xyz);
    LPD_CHECK_ARG(sel != 0 && sel < (1u << LPD_FEAT_COLUMNS), "lpd_local_features: sel=0x%x selects no column or one past the %d defined",
                  sel, LPD_FEAT_COLUMNS);
    const int width = (copy_xyz ? 3 : 0) + __builtin_popcount(sel);
    LPD_CHECK_ARG(ldo >= width, "lpd_local_features: ldo=%d is smaller than the %d columns of a row", ldo, width);
    LPD_CHECK_ARG((const void*)out != (const void*)xyz, "lpd_local_features: out must not alias xyz");
    LPD_CHECK_ARG(ncand >= 0 && ncand <= 16, "lpd_local_features: ncand=%d (at most 16 candidate sizes)", ncand);
    unsigned long long evalmask = 0;
    int kmax = K;
    if (cand && ncand > 0) {
        int prev = 3;
        for (int c = 0; c < ncand; ++c) {
            LPD_CHECK_ARG(cand[c] > prev && cand[c] <= K, "lpd_local_features: candidate sizes must be strictly ascending in [4, K=%d] (cand[%d]=%d)",
                          K, c, (int)cand[c]);
            prev = cand[c];
            evalmask |= 1ull << (cand[c] - 1);
        }
        kmax = prev;
    } else evalmask = 1ull << (K - 1);
    // A/B switch, read on every call (a test flips it inside one process): LPD_DEBUG=feat-l2 sends every cloud through the L2 form
    const bool lds = N <= FEAT_LDS_MAX_N && !lpd_debug("feat-l2", 0);
    const int T = lds ? FEAT_T_LDS : FEAT_T_L2;
    const long long blocks = (long long)B * ((N + T - 1) / T);
    LPD_CHECK_ARG(blocks < (1ll << 31), "lpd_local_features: grid of %lld blocks", blocks);
    const int vec4 = (K % 4 == 0 && ((uintptr_t)idx & 15) == 0) ? 1 : 0;
    if (lds)
        hipLaunchKernelGGL(local_features_kernel<true>, dim3((unsigned)blocks), dim3(T), (size_t)N * 3 * sizeof(float), stream, xyz, ldx, idx,
                           N, K, kmax, evalmask, sel, copy_xyz, out, ldo, kopt, vec4);
    else
        hipLaunchKernelGGL(local_features_kernel<false>, dim3((unsigned)blocks), dim3(T), 0, stream, xyz, ldx, idx, N, K, kmax, evalmask,
                           sel, copy_xyz, out, ldo, kopt, vec4);
    LPD_CHECK_LAUNCH("lpd_local_features");
    return LPD_OK;
}
