// lpd_feat.hip -- local point-distribution features: the five handcrafted per-point columns behind xyz that the use_mFea trunks
// of LPD-Net take (reference lpdnet_model.py:183-186,215-224 reads them from an offline preprocessing step), computed on the device
// from each point's sorted kNN list.  Definition of the ten columns: include/lpd_hip.h; arithmetic: lpd_feat_math.h.
//
// One lane per point.  The lane walks its list ONCE, nearest first, accumulating the moments of d_j = x_{n_j} - x_i; the candidate
// neighbourhood sizes of the adaptive form are prefixes of that walk: after the k-th entry of a candidate size k the lane solves the
// 3x3 eigenproblem of the moments so far and keeps them when their eigenentropy is the smallest yet.  The candidate sizes arrive as a
// 64-bit mask (bit k-1 = "evaluate after k entries"; K <= 64), a kernel argument -- no device copy of the host array.
//
// The walk itself -- the two forms of the neighbour read (cloud in LDS, or through L2), the staging, the list read and the clamp -- is
// lpd_list_walk.h, shared with point_normals_kernel (lpd_icp.hip).  What is here: the moments, the candidates, the columns.
#include "lpd_common.h"
#include "lpd_feat_math.h"
#include "lpd_list_walk.h"

namespace {

template <bool LDS>
__global__ __launch_bounds__(lpd_walk_threads<LDS>) void local_features_kernel(
    const float* __restrict__ xyz, int ldx, const int32_t* __restrict__ idx, int N, int K, int kmax, unsigned long long evalmask,
    unsigned sel, int copy_xyz, float* __restrict__ out, int ldo, int32_t* __restrict__ kopt, int vec4)
{
    LpdListWalk w;
    if (!lpd_walk_open<LDS>(w, xyz, ldx, idx, N, K)) return;
    LpdFeatMoments m, best;
    lpd_feat_init(m);
    best = m;
    float best_a = INFINITY;
    int best_k = 0;
    lpd_walk<LDS, false>(w, kmax, vec4, [&](int j, float dx, float dy, float dz) {
        lpd_feat_add(m, dx, dy, dz);
        if ((evalmask >> j) & 1ull) {      // a candidate size ends here (uniform: the mask is a kernel argument)
            const float a = lpd_feat_entropy(lpd_feat_eig(lpd_feat_cov(m, j + 1)));
            if (a < best_a) {              // strict: ties go to the smaller size
                best_a = a;
                best = m;
                best_k = j + 1;
            }
        }
    });
    float f[LPD_FEAT_COLUMNS];
    lpd_feat_columns(best, best_k, f);
    const size_t mrow = w.mrow();
    float* o = out + mrow * ldo;
    int col = 0;
    if (copy_xyz) {
        o[0] = w.px;
        o[1] = w.py;
        o[2] = w.pz;
        col = 3;
    }
#pragma unroll
    for (int c = 0; c < LPD_FEAT_COLUMNS; ++c)
        if ((sel >> c) & 1u) o[col++] = f[c];
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
    const LpdWalkPlan plan = lpd_walk_plan(idx, B, N, K, lpd_debug("feat-l2", 0) != 0);
    LPD_CHECK_ARG(plan.blocks < (1ll << 31), "lpd_local_features: grid of %lld blocks", plan.blocks);
    hipLaunchKernelGGL(plan.lds ? local_features_kernel<true> : local_features_kernel<false>, dim3((unsigned)plan.blocks), dim3(plan.threads),
                       plan.lds_bytes, stream, xyz, ldx, idx, N, K, kmax, evalmask, sel, copy_xyz, out, ldo, kopt, plan.vec4);
    LPD_CHECK_LAUNCH("lpd_local_features");
    return LPD_OK;
}
