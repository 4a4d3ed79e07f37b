/*
 * include/lpd_hip.h -- C-ABI of liblpd_hip.so, the MI355X (gfx950) kernels of the LPD-Net
 * global-descriptor hot path.
 *
 * The reference (qiaozhijian/LPD-Net-Pytorch) is pure Python and has no FFI layer of its own; the
 * drop-in boundary is its Python module API (util.PointNetVlad / util.lpdnet_model /
 * loss.pointnetvlad_loss), mirrored by lpd-net-pytorch_amd/.  This header is the boundary UNDER
 * that mirror: each entry point names the reference lines it replaces.  A maintainer binds it with
 * ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain C: device pointers, ints, floats; no torch types, no exceptions.
 *   - the caller owns every buffer (inputs, outputs, workspaces); nothing here allocates.  Entry points that reduce over
 *     workgroups (BatchNorm statistics and their backward sums) take `double* stat_ws`: lpd_stat_ws_bytes() bytes of device
 *     memory, zero-filled ONCE by the caller; every call that returns LPD_OK leaves it all-zero again, so one workspace serves
 *     all calls on one stream (two streams that run concurrently need two).  After an LPD_ERR_LAUNCH return re-zero it.
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream); nothing synchronises.
 *   - return 0 on success, <0 on error (LPD_ERR_*); lpd_last_error() gives the text
 *     (thread-local).  No global mutable state => callable concurrently from several host
 *     threads (nn.DataParallel-style callers) on different streams/devices.
 *   - all tensors fp32 unless noted; "point-major" = [rows = B*N points][channels], row-major;
 *     "channel-major" = the reference's [B][C][N].
 *   - activation codes: 0 none, 1 ReLU, 2 LeakyReLU(slope), 3 sigmoid.
 */
/*
 * Entry points that are NOT on a default path (tools/abi_coverage.py, profiles/r06_abi_coverage.txt: eval forwards and train steps of
 * every trunk in both storage modes and both product modes, ragged cloud sizes, the callers' helpers -- 81 of the 101 entry points
 * are called, 3 more are infrastructure: lpd_version, lpd_last_error, lpd_knn_pm_layout).  The 17 below are SUPERSEDED formulations,
 * kept because tests use them as on-device cross-checks of the fused kernels that replaced them; the Python mirror reaches them only
 * through an LPD_DEBUG token.  A binding that wants the product path does not need them:
 *   lpd_gemm_bf16x1                      one bf16 product per term (LPD_DEBUG=bf16-x1)
 *   lpd_split_panels                     fp32 panels -> split bf16 planes as a pass of its own (the producers write planes)
 *   lpd_edge_gather_max                  K-agg with every gather through L2 (superseded by the cloud-resident / windowed kernels)
 *   lpd_group_max, lpd_group_max_bwd, lpd_scatter_add_rows, lpd_edge_split_fwd (wave-per-point form)
 *                                        materialised [M k, C] edge tensors of rounds 1-2 (the split-form stage works from gather sums)
 *   lpd_edge_build_bf16, lpd_edge_act_max_bf16, lpd_group_sel_stats_bf16, lpd_edge_bn_bwd_bf16, lpd_edge_bn_bwd_bf16_sel,
 *   lpd_gemm_bf16s, lpd_gemm_bf16s_bnbwd, lpd_gather_sum_rows_bf16
 *                                        round 3's chain of passes for the bf16-storage DG1 -> DG2 stage (one launch forward, two backward now)
 *   lpd_gemm_tn_bf16 (+ _ws_floats)      weight gradients on the register-transposing kernel (superseded by the transposed-read kernel)
 * The kNN `impl` values 1 / 2 / 4 / 6 of lpd_knn are test cross-checks and A/B timing forms as well (see lpd_knn below).
 */
#ifndef LPD_HIP_H
#define LPD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LPD_OK 0
#define LPD_ERR_ARG (-1)
#define LPD_ERR_LAUNCH (-2)
#define LPD_ERR_UNSUPPORTED (-3)

#define LPD_ACT_NONE 0
#define LPD_ACT_RELU 1
#define LPD_ACT_LEAKY 2
#define LPD_ACT_SIGMOID 3

int lpd_version(void);
const char* lpd_last_error(void);
/* size of the `stat_ws` workspace (see Conventions): 32 replicas x 2 x LPD_STAT_CMAX doubles = 512 KiB; a layer of more columns is
 * refused by the entry points that take it */
#define LPD_STAT_CMAX 1024
long long lpd_stat_ws_bytes(void);

/*
 * kNN graph construction.  Replaces util/lpdnet_model.py:317-326 `knn(x, k)`.
 *   x      [B][C][N] channel-major (exactly the reference's argument layout)
 *   idx    [B][N][k] int32, the k largest pd = -|x_i - x_j|^2 (reference arithmetic order, see
 *          csrc/lpd_knn.hip), descending; self is included; ties -> lower index first.
 *   ws     workspace of lpd_knn_workspace_floats(B, C, N, k) floats: per-point sums of squares, the packed MFMA operand
 *          image xp[b][n][h][s] = x[b][2s+h][n], and (best-first path) per-tile centroids / radii / visiting orders
 *   impl   0 = product path: f32-MFMA distance tiles + queued selection; best-first tile order with exact skip bounds for
 *          C <= 64, k <= 64 (four waves per query tile while the grid would not fill the chip), the first-generation kernel for
 *          64 < C <= 256.  Everything else is NOT a product path: 4 / 6 = ascending scan / best-first walk forced (A/B timing, same
 *          indices), 5 = per-wave walk statistics INSTEAD of indices (tools/knn7_stats.py), 1 = VALU fmaf cross-check of the MFMA
 *          arithmetic (k <= 20; an on-device oracle for tests), 2 = first-generation kernel forced.  Other values: LPD_ERR_ARG.
 *          (impl 3 and the timing ablations 10..137 of rounds 1-2 were removed in round 5.)
 * Supported: C <= 256, k <= 64, k <= N.  Bit-exact vs the reference CPU path on tie-free rows.
 */
int lpd_knn(const float* x, int B, int C, int N, int k, int32_t* idx, float* ws, int impl, void* stream);
long long lpd_knn_workspace_floats(int B, int C, int N, int k);
/* The same on point-major rows x_pm [B*N][ld] (the pipeline's activation layout; C <= 64, k <= 64): no transposes. */
int lpd_knn_pm(const float* x_pm, int ld, int B, int C, int N, int k, int32_t* idx, float* ws, int impl, void* stream);
/* impl | LPD_KNN_PM_PREPARED: the operands of the 64-channel cloud are in ws already (lpd_lpdnet_front wrote them); x_pm may be
 * NULL.  lpd_knn_pm_layout: where lpd_knn_pm keeps them -- squared norms xx [B*N], packed operand image xp [B*N][2][32], the
 * bf16 image xb of the low-precision bound pass (NULL unless that pass will run on these sizes AND takes the image from whoever
 * writes the operands: C = 64, N % 32 == 0; elsewhere the search makes it itself) and the statistics of the
 * 32-point tiles of the best-first search (centroids [B*nt][2 cp] in packed operand order, then |c|^2, radius and max |x|^2,
 * [B*nt] each; nt = ceil(N / 32), cp = 2 for C <= 4 else 32; NULL when the best-first search will not run).  "Prepared" means
 * all of these. */
#define LPD_KNN_PM_PREPARED 256
/* (C = 3, N % 32 == 0: lpd_morton_sort_knn prepares the workspace of the xyz search the same way.) */
int lpd_knn_pm_layout(int B, int C, int N, int k, float* ws, float** xx, float** xp, void** xb, float** tiles);
/* Default path (the xyz graph of the LPD-Net eval forward): lpd_knn_pm whose lists also leave as the blocked uint16 copy that
 * lpd_pack_idx16 makes (k = 20, N % 32 == 0; idx16 [B*N][20] uint16, 16-byte aligned), bit for bit.  Where lpd_knn_pm16_fused(C, N, k,
 * impl) is 1 the search's final merge writes the 1280-byte blocks itself -- a wave's 32 queries are exactly one block -- and idx may be
 * NULL (no int32 lists are written); elsewhere (the ascending scan, the branchy / statistics variants, LPD_DEBUG=knn-pack16=0) idx is
 * required and lpd_pack_idx16 runs behind the search as a launch of its own. */
int lpd_knn_pm16_fused(int C, int N, int k, int impl);
/* Infrastructure: the byte offset of neighbour s (0 .. 19) of row m inside the blocked uint16 lists (the address arithmetic of the
 * search's packed store; host only, -1 for arguments out of range). */
long long lpd_idx16_offset(long long m, int s);
int lpd_knn_pm16(const float* x_pm, int ld, int B, int C, int N, int k, int32_t* idx, uint16_t* idx16, float* ws, int impl, void* stream);

/*
 * The layers in front of the feature-space kNN of LPD-Net in one launch (util/lpdnet_model.py:231-232, no T-Nets):
 *   F0 = act(BN2(conv2_lpd(act(BN1(conv1_lpd(xyz))))))   xyz [B*N][ldx] (3 coordinates used), W1 [64][3], W2 [64][64] ([out][in]),
 *   s / b = folded eval-mode BatchNorm scale / shift, act none / ReLU / LeakyReLU; exact fp32 (fma chains, f32-input MFMA).
 * F0 [B*N][64] row-major.  knn_ws != NULL (a lpd_knn_workspace_floats(B, 64, N, k) workspace): the kNN operands of F0 are
 * written there too, and lpd_knn_pm(NULL, 64, B, 64, N, k, idx, knn_ws, LPD_KNN_PM_PREPARED, stream) builds the graph.
 * N % 128 == 0.
 */
int lpd_lpdnet_front(const float* xyz, int ldx, const float* W1, const float* s1, const float* b1, const float* W2, const float* s2,
                     const float* b2, int act, float slope, float* F0, int B, int N, int k, float* knn_ws, void* stream);

/*
 * Dense fp32 GEMM with fused epilogue:  C = act((A.B + bias) * scale + shift), per output column.
 * Replaces the 1x1 Conv1d/Conv2d + eval BatchNorm + activation stacks
 * (util/lpdnet_model.py:231-232,262,297-305; util/PointNetVlad.py:152-175,213-230), the NetVLAD
 * matmuls (PointNetVlad.py:48,66,76) and the gating matmul (PointNetVlad.py:104).
 *   A logical [M][K]: a_kmajor = 0 -> stored [M][lda]; 1 -> stored [K][lda] (i.e. A^T in memory)
 *   B logical [K][N]: b_kmajor = 1 -> stored [K][ldb]; 0 -> stored [N][ldb] (torch conv weight)
 *   batch > 1: strides sA/sB/sC in elements between problems
 *   splits > 1: split-K; splitk_ws must hold batch*splits*M*N floats; epilogue applied after the sum
 *   bias/scale/shift: [N] or NULL (scale and shift together)
 *   accumulate != 0: C += result (after the epilogue) -- gradient accumulation in the backward pass
 * Any M, N, K (tails are zero-filled / masked).  Requires lda/ldb/sA/sB % 4 == 0, A and B 16-byte aligned.
 *   a_cloud / c_cloud != 0: A / C are in CLOUD-PANEL layout [cloud][cols/8][panel_ld][8] (lda / ldc ignored): rows
 *   m = cloud * panel_n + n, n < panel_n <= panel_ld (the pad rows keep consecutive panels off the same HBM channels);
 *   a_cloud / c_cloud = floats between clouds of that buffer (it may hold more panels than the operand uses: pass the
 *   pointer to the operand's first panel).  An 8-channel slice of one cloud is one contiguous
 *   32*panel_n-byte run -- what lpd_edge_gather_max16 streams -- and a whole cloud one contiguous block.  Needs
 *   a_kmajor = 0, batch = 1, splits = 1, K % 32 == 0, panel_n % 128 == 0.
 */
int lpd_gemm(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
             int a_kmajor, int b_kmajor, int batch, long long sA, long long sB, long long sC, int splits,
             float* splitk_ws, const float* bias, const float* scale, const float* shift, int act, float slope,
             int accumulate, long long a_cloud, long long c_cloud, int panel_n, int panel_ld, void* stream);

/*
 * lpd_gemm on the bf16 MFMA: each fp32 operand is split hi + lo (two bf16) while it is staged into LDS and every
 * product is the sum of three bf16 MFMA products (a_lo*b_hi + a_hi*b_lo + a_hi*b_hi), fp32 accumulation.  Error
 * ~5e-6 of the output range (the f32-input form: ~5e-7); 2e-6 on the final descriptors (DESIGN.md "GEMM precision").
 * Same arguments and layouts as lpd_gemm.
 */
int lpd_gemm_bf16x3(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
             int a_kmajor, int b_kmajor, int batch, long long sA, long long sB, long long sC, int splits,
             float* splitk_ws, const float* bias, const float* scale, const float* shift, int act, float slope,
             int accumulate, long long a_cloud, long long c_cloud, int panel_n, int panel_ld, void* stream);

/* The same kernel with ONE product per term (a_hi * b_hi: the operands rounded to bf16, fp32 accumulation): the bf16-storage
 * training mode (BASELINE.json configs[2]).  ~4e-3 relative per operand. */
int lpd_gemm_bf16x1(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
             int a_kmajor, int b_kmajor, int batch, long long sA, long long sB, long long sC, int splits,
             float* splitk_ws, const float* bias, const float* scale, const float* shift, int act, float slope,
             int accumulate, long long a_cloud, long long c_cloud, int panel_n, int panel_ld, void* stream);

/*
 * Split-bf16 GEMM for a weight-shaped B: lpd_gemm_prep_b splits B (either layout) once into hi/lo bf16 stored in MFMA
 * fragment order (lpd_gemm_prep_b_bytes(N, K) bytes, 16-byte aligned); lpd_gemm_x3w then computes
 * C = act((A.B + bias) * scale + shift) for row-major A [M][lda] without staging or splitting B again (each wave streams
 * its 32-column fragments from L2 into registers).  Used for the wide forward layers (conv3 512 -> 1024, the split edge
 * projections) and for dX = dY.W in the backward pass.  a_cloud / c_cloud / panel_n / panel_ld: cloud-panel A / C as in
 * lpd_gemm (0 = row-major).  impl: 0 = by shape (N >= 256: 128 x 256 blocks, each wave a 128 x 64 strip; else 128 x 128),
 * 2 / 3 = 128 x 128 / 128 x 256 blocks forced; impl | 16: one product per term (a_hi * b_hi, see lpd_gemm_bf16x1).
 */
long long lpd_gemm_prep_b_bytes(int N, int K);
int lpd_gemm_prep_b(const float* B, int ldb, int b_kmajor, int N, int K, void* frags, void* stream);
/* `batch` matrices sB floats apart -> `batch` fragment sets lpd_gemm_prep_b_bytes(N, K) bytes apart (lpd_gemm_x3t_rows, batched) */
int lpd_gemm_prep_b_batch(const float* B, int ldb, int b_kmajor, int N, int K, int batch, long long sB, void* frags, void* stream);
int lpd_gemm_x3w(const float* A, int lda, const void* frags, float* C, int ldc, int M, int N, int K, const float* bias,
                 const float* scale, const float* shift, int act, float slope, int accumulate,
                 long long a_cloud, long long c_cloud, int panel_n, int panel_ld, int impl, void* stream);

/* The bare product C = A W^T (+ bias) of a TRAIN-mode layer with its BatchNorm statistics from the epilogue: stat_sum / stat_sumsq
 * [N] fp64 (zeroed by the call) = column sums / sums of squares of C over the M rows (fp32 over a block's 128 rows, fp64 atomics),
 * i.e. lpd_colstats without the second pass over C. */
/* lpd_gemm_x3w with per-problem weights: rows [b batch_rows, (b + 1) batch_rows) of the row-major A take fragment set b of
 * lpd_gemm_prep_b_batch (frag_bytes = lpd_gemm_prep_b_bytes(N, K) apart); batch_rows % 128 == 0.  NetVLAD backward's dA[b] = x[b] . dV[b]. */
/* a_scale / a_shift (or null): the rows of A are act(a_scale[k] A[m][k] + a_shift[k]) -- lpd_gemm_x3w_act's operand transform with
 * nothing stored (bf16 rows: the transformed values rounded to bf16 = the map a bf16-storing lpd_gemm_x3w_act writes) */
int lpd_gemm_x3w_batched(const void* A, int lda, int a_bf16, const void* frags, long long frag_bytes, int batch_rows, float* C, int ldc, int M,
                         int N, int K, const float* a_scale, const float* a_shift, int a_act, float a_slope, int impl, void* stream);
/* bf16 rows as the operand (a_bf16 above, flags & 1 of lpd_gemm_x3w_act, lpd_gemm_x3w_bf16a): A [M][lda] in bf16 elements, row-major,
 * K % 32 == 0.  A plain product takes the rows as the hi image (two MFMA products against the split weight); with an operand
 * transform they are widened first.  flags & 2 of lpd_gemm_x3w_act: a_out is a bf16 tensor, and the product sees the rounded values.
 * The bf16-storage training mode keeps the [B N, 1024] conv3 map, its activated form and its gradient as bf16. */
int lpd_gemm_x3w_bf16a(const void* A16, int lda, const void* frags, float* C, int ldc, int M, int N, int K, int accumulate, int impl, void* stream);
/* c_bf16 & 1: C receives bf16 values ([M][ldc] in bf16 elements, N % 32 == 0); the statistics stay those of the fp32 accumulators.
 * c_bf16 & 2: A holds bf16 rows too (lda in bf16 elements, K % 32 == 0; with a bf16 C and N >= 256): two products per term */
int lpd_gemm_x3w_stats(const float* A, int lda, const void* frags, void* C, int ldc, int c_bf16, int M, int N, int K, const float* bias,
                       double* stat_sum, double* stat_sumsq, int impl, double* stat_ws, void* stream);
/* The product with the train-mode BatchNorm affine + activation of the layer IN FRONT applied in the operand loader:
 * C = act(a_scale[k] A[m][k] + a_shift[k]) W^T (+ bias), the transformed rows stored to a_out [M][a_ld] on the way (or null).
 * Row-major A, N <= 128.  util/lpdnet_model.py:262 (bn3_lpd + act) feeding util/PointNetVlad.py:48 (x . cluster_weights): the
 * stand-alone affine pass over the [B N, 1024] map disappears.  impl: 0, or 16 = plain bf16 operands (bf16 storage mode). */
int lpd_gemm_x3w_act(const void* A, int lda, const void* frags, float* C, int ldc, int M, int N, int K, const float* bias,
                     const float* a_scale, const float* a_shift, int a_act, float a_slope, void* a_out, int a_ld, int flags, int impl, void* stream);

/*
 * The same product for a SHORT reduction with cloud-panel A and C (the neighbour / centre projection of the split SN1 edge
 * convolution, util/lpdnet_model.py:257: K = 128 -> N = 512), computed transposed: the prepared weight fragments are the MFMA's
 * row operand, each wave keeps its 32 data rows (split hi / lo once) in registers for all N columns and stores whole KiB runs of
 * a panel -- no LDS, no barrier.  lpd_gemm_x3t_applies: K in {64, 128}, N % 32 == 0, both operands cloud panels, clouds of a
 * multiple of 128 points, act none / ReLU / LeakyReLU.  frags: lpd_gemm_prep_b(W [N][K], b_kmajor = 0).
 */
int lpd_gemm_x3t_applies(int M, int N, int K, int act, long long a_cloud, long long c_cloud, int panel_n);
/* lpd_gemm_x3t with A given as SPLIT bf16 planes (a_hi: hi plane [cloud][K/8][panel_ld][8], a_cloud elements between clouds; the lo
 * plane a_lo elements behind it) */
int lpd_gemm_x3ts(const void* a_hi, long long a_lo, const void* frags, float* C, int M, int N, int K, const float* bias,
                  const float* scale, const float* shift, int act, float slope, long long a_cloud, long long c_cloud, int panel_n,
                  int panel_ld, void* stream);
/* The transposed short-reduction product on ROW-MAJOR fp32 operands: C [M][ldc] = act((A [M][lda] . W^T + bias) * scale + shift) with the
 * fragments of lpd_gemm_prep_b; K = 64 or 128, N % 32 == 0, M % 128 == 0.  batch > 1: independent problems with their own A, C
 * (strides sA, sC in floats) and fragment sets (frag_bytes apart). */
int lpd_gemm_x3t_rows_applies(int M, int N, int K, int act, long long lda, long long ldc);
/* c_bf16: C receives bf16 values (ldc / sC in bf16 elements, ldc % 8 == 0) */
int lpd_gemm_x3t_rows(const float* A, long long lda, const void* frags, void* C, long long ldc, int c_bf16, int M, int N, int K, const float* bias,
                      const float* scale, const float* shift, int act, float slope, int batch, long long sA, long long sC,
                      long long frag_bytes, void* stream);

int lpd_gemm_x3t(const float* A, const void* frags, float* C, int M, int N, int K, const float* bias, const float* scale,
                 const float* shift, int act, float slope, long long a_cloud, long long c_cloud, int panel_n, int panel_ld,
                 void* stream);

/*
 * kNN-graph aggregation (K-agg).  Replaces the gather/repeat/cat of util/lpdnet_model.py:331-363
 * fused with a split edge convolution + BatchNorm + activation + max over k
 * (lpdnet_model.py:249-250 convDG1/x1, :257-258 convSN1/x3):
 *   out[m][c] = act(scale[c] * (sel_t P[cloud(m)*N + idx[m][t]][c] + Q[m][c]) + shift[c])
 *   sel = max over the k neighbours where scale[c] >= 0, min where scale[c] < 0.
 *   P [M][ldp], Q [M][ldq] or NULL, idx [M][k] (indices local to the cloud), out [M][ldo].
 * C in {64,128,256}; M = B*N; leading dims % 4 == 0; pointers 16-byte aligned.
 */
int lpd_edge_gather_max(const float* P, int ldp, const float* Q, int ldq, const int32_t* idx, float* out, int ldo,
                        const float* scale, const float* shift, int M, int N, int C, int k, int act, float slope,
                        void* stream);

/*
 * K-agg, cloud-resident form on row-major operands with 16-bit indices: as lpd_edge_gather_max, but one
 * workgroup keeps an 8-channel slice of ALL N rows of one cloud's P in LDS (N*32 bytes), so the k gathers per
 * point are LDS reads and P, Q, out cross the memory system once.  idx16: the blocked uint16 copy made by lpd_pack_idx16.
 * Built for k = 20, N <= 4096; bit-identical to lpd_edge_gather_max.
 * p_cloud / q_cloud / o_cloud != 0: that operand is in cloud-panel layout [cloud][.][panel_ld][8] (floats between clouds; leading
 * dim ignored): a block's 8-channel slice is then one contiguous 32*N-byte run instead of N pieces of 32 bytes.
 */
int lpd_edge_gather_max16(const float* P, int ldp, const float* Q, int ldq, const uint16_t* idx16, float* out, int ldo,
                          const float* scale, const float* shift, int M, int N, int C, int k, int act, float slope, long long p_cloud,
                          long long q_cloud, long long o_cloud, int panel_ld, void* stream);
/* The same with SPLIT output for lpd_gemm_p8 / lpd_gemm_x3ts: out_hi = hi plane of a pair of bf16 cloud-panel planes
 * [cloud][C/8][panel_ld][8] (hi = bf16(x), lo = bf16(x - hi); o_cloud bf16 elements between clouds), the lo plane o_lo elements
 * behind it.  Same bytes as the fp32 row; the two lanes of a point exchange halves (DPP) so that each still stores 16 bytes. */
int lpd_edge_gather_max16s(const float* P, int ldp, const float* Q, int ldq, const uint16_t* idx16, void* out_hi, long long o_lo,
                           const float* scale, const float* shift, int M, int N, int C, int k, int act, float slope, long long p_cloud,
                           long long q_cloud, long long o_cloud, int panel_ld, void* stream);

/* int32 kNN indices [M][k] (local to the cloud, < 65536) -> the uint16 copy lpd_edge_gather_max16 reads:
 * blocked by 32 points, index quad i of point m at ((m/32)*5 + i)*32 + m%32 (uint2 units); idx16 holds
 * ceil(M/32)*32*k uint16.  k = 20. */
int lpd_pack_idx16(const int32_t* idx, uint16_t* idx16, long long M, int k, void* stream);

/*
 * K-agg for LARGE clouds (N > 4096, e.g. BASELINE configs[4]: N = 16384, k = 64): a Z-order WINDOW of 4095 rows of the cloud's
 * 8-channel slice in LDS, neighbours outside the window from L2 (csrc/lpd_edge_win.hip).  Same result, bit for bit, as
 * lpd_edge_gather_max; operands as lpd_edge_gather_max16 (row-major or cloud-panel).  idx16: the RAW uint16 copy of the
 * indices made by lpd_pack_idx16w (blocked by 32 points, quad i of point m at ((m/32)*(k/4) + i)*32 + m%32, uint2 units;
 * ceil(M/32)*32*k uint16).  k in {20, 32, 64}; N <= 57344; the clouds should be Z-ordered (lpd_morton_sort) for the window to
 * catch most neighbours -- correctness does not depend on it.  lpd_pack_idx16w with N > 0 (points per cloud) also PARTITIONS every
 * list, out-of-window neighbours first (the miss phase then stops at the longest miss list of a wave); N = 0 keeps the kNN order.
 */
int lpd_pack_idx16w(const int32_t* idx, uint16_t* idx16, long long M, int k, int N, void* stream);
int lpd_edge_gather_maxw(const float* P, int ldp, const float* Q, int ldq, const uint16_t* idx16, float* out, int ldo,
                         const float* scale, const float* shift, int M, int N, int C, int k, int act, float slope, long long p_cloud,
                         long long q_cloud, long long o_cloud, int panel_ld, void* stream);

/*
 * Fused per-edge MLP: stage-1 BatchNorm+activation on the fly, stage-2 1x1 conv on the f32 MFMA,
 * BatchNorm + activation + max over k.  Replaces util/lpdnet_model.py:251-252 (convDG2 applied to
 * the un-maxed convDG1 output, then max) and the LPDNetOrign chains lpdnet_model.py:97-100,105-107:
 *   y1[m][t][:] = act(s1 * (P[nbr(m,t)] + Q[m]) + b1)            (never materialised)
 *   out[m][o]   = act(s2[o] * sel_t (W2 y1[m][t])[o] + b2[o])
 *   W2 [CO][CM] torch [out,in] layout.  (CM,CO) in {(128,128),(64,64)}; k <= 128.
 *   out_cloud != 0: out is in cloud-panel layout [cloud][.][panel_ld][8] with out_cloud floats between clouds (ldo ignored).
 */
int lpd_edge_mlp(const float* P, int ldp, const float* Q, int ldq, const int32_t* idx, const float* s1,
                 const float* b1, const float* W2, const float* s2, const float* b2, float* out, int ldo, int M,
                 int N, int CM, int CO, int k, int act, float slope, long long out_cloud, int panel_ld, void* stream);
/* Same contract on the bf16 MFMA (split-bf16, three products per term, fp32 accumulate: see lpd_gemm_bf16x3). */
int lpd_edge_mlp_bf16x3(const float* P, int ldp, const float* Q, int ldq, const int32_t* idx, const float* s1,
                 const float* b1, const float* W2, const float* s2, const float* b2, float* out, int ldo, int M,
                 int N, int CM, int CO, int k, int act, float slope, long long out_cloud, int panel_ld, void* stream);
/* ... with SPLIT output (see lpd_edge_gather_max16s): out_hi / out_lo planes of bf16 cloud panels, out_cloud elements between clouds */
int lpd_edge_mlp_bf16x3s(const float* P, int ldp, const float* Q, int ldq, const int32_t* idx, const float* s1,
                 const float* b1, const float* W2, const float* s2, const float* b2, void* out_hi, long long out_lo, int M,
                 int N, int CM, int CO, int k, int act, float slope, long long out_cloud, int panel_ld, void* stream);
/* ... and with x1 = max over k of the stage-1 activation act(s1 (P_j + Q_i) + b1) -- the DG1-stage K-agg of LPDNet.forward
 * (util/lpdnet_model.py:249-250), which is the maximum over the slots of the very tile this kernel builds for the DG2 product --
 * written on the way as a second pair of planes (x1_hi, x1_hi + out_lo; layout of out_hi): one launch instead of lpd_pack_idx16 +
 * lpd_edge_gather_max16s + lpd_edge_mlp_bf16x3s over the same graph.  128 -> 128 channels, M % 32 == 0, N % 64 == 0. */
int lpd_edge_mlp_x1_bf16x3s(const float* P, int ldp, const float* Q, int ldq, const int32_t* idx, const float* s1,
                 const float* b1, const float* W2, const float* s2, const float* b2, void* out_hi, void* x1_hi, long long out_lo,
                 int M, int N, int k, int act, float slope, long long out_cloud, int panel_ld, void* stream);

/* Per-point linear layer with K <= 8 inputs (+bias, affine, activation): the 3 -> 64 first layers
 * (util/lpdnet_model.py:185,231; util/PointNetVlad.py:190,213; T-Net conv1 lpdnet_model.py:276) and the
 * per-cloud 3x3 alignment products x @ trans (lpdnet_model.py:229; PointNetVlad.py:209).
 * Weight element (n, c) of weight set b is W[b*w_sb + n*w_sn + c*w_sk]; row m uses set m / rows_per_w
 * (rows_per_w = 0: one shared weight). */
int lpd_linear_smallk(const float* X, int ldx, const float* W, int w_sn, int w_sk, long long w_sb, int rows_per_w,
                      float* Y, int ldy, int M, int N, int K, const float* bias, const float* scale,
                      const float* shift, int act, float slope, void* stream);

/* Batched transpose in [batch][R][C] -> out [batch][C][R] (point-major <-> channel-major). */
int lpd_transpose(const float* in, float* out, int batch, int R, int C, int ldi, int ldo, long long si,
                  long long so, void* stream);

/* NetVLAD soft-assignment: out[r][:] = softmax(scale * in[r][:] + shift), ncols <= 64
 * (util/PointNetVlad.py:51-58, eval-mode bn1 folded into scale/shift). In-place allowed.
 * colsum != NULL: rows come in groups (clouds) of group_rows (a multiple of 16) and colsum[g * colsum_ld + c] receives
 * (=) the column sums of `out` over group g -- NetVLAD's a_sum (:63) without a second pass over the assignments; the other
 * colsum_ld - ncols entries of row g are set to 0.  part: scratch of rows / 16 * 64 floats for the partial sums, which a
 * second launch adds in a fixed order (no float atomics: the same input gives the same bits in every launch). */
int lpd_softmax_affine(const float* in, float* out, int rows, int ncols, const float* scale, const float* shift,
                       int group_rows, float* colsum, int colsum_ld, float* part, void* stream);

/* NetVLAD residual + normalisations (util/PointNetVlad.py:61-74).
 *   vraw [B][F][KC] = act^T x per cloud, act [B][N][KC], cw2 [F][KC] (cluster_weights2[0]),
 *   out [B][F*KC]: (vraw - a_sum*cw2), L2-normalised over F per cluster, flattened f*KC+c, L2-normalised. KC = 64.
 *   ws: workspace of B*2*KC floats, ws[b][0..KC) = a_sum (written here); asum_ready != 0: ws[b][0..KC) already holds a_sum
 *   (lpd_softmax_affine with colsum = ws, colsum_ld = 2*KC), act may be NULL.  ws[b][KC..2KC) is not touched.
 *   part: scratch of B*(16 + ceil(F/64))*KC floats: per-block partial sums of a_sum and of the per-cluster sums of squares,
 *   added by their readers in block order (no float atomics: the same input gives the same bits in every launch).
 *   aux_asum [B][KC], aux_inv_c [B][KC], aux_inv_g [B]: optional (NULL in inference) -- a_sum and the two
 *   reciprocal norms, saved for lpd_vlad_finalize_bwd. */
int lpd_vlad_finalize(const float* vraw, const float* act, const float* cw2, float* out, float* ws, float* part, float* aux_asum,
                      float* aux_inv_c, float* aux_inv_g, int B, int N, int F, int KC, int asum_ready, void* stream);

/* Per-cloud max over the N points: in [B][N][ldi] -> out [B][C]
 * (util/PointNetVlad.py:137,162 mp1; util/lpdnet_model.py:300). */
int lpd_colmax(const float* in, int ldi, float* out, int B, int N, int C, void* stream);

/* Context gating in one launch (util/PointNetVlad.py:103-115): out[b][:] = h[b][:] * sigmoid((h[b][:] . Wg + bias) * scale + shift),
 * h [B][ldh], Wg [D][ldw] (gating_weights, k-major), bias / (scale, shift) optional per-column vectors (the eval-mode bn1
 * affine or gating_biases).  out may not alias h. */
int lpd_gating(const float* h, int ldh, const float* Wg, int ldw, const float* bias, const float* scale, const float* shift,
               float* out, int ldo, int B, int D, void* stream);

/* out = a * b elementwise (context gating product, util/PointNetVlad.py:113). */
int lpd_mul(const float* a, const float* b, float* out, long long n, void* stream);

/*
 * Lazy triplet / quadruplet loss, forward + gradient in one launch.  Replaces
 * loss/pointnetvlad_loss.py:6-97 (best_pos_distance, triplet_loss, quadruplet_loss).
 *   q (b,0,d) at q[b*q_sb + d]; pos (b,p,d) at pos[b*pos_sb + p*pos_st + d]; neg likewise; other like q
 *   (strides in elements, unit stride over d) -- the four inputs are normally views of one
 *   [bq, 1+P+Ng+1, D] descriptor tensor (train_pointnetvlad.py:214-217).
 *   quad = 0: triplet form (other/m2/gother ignored).  use_min / lazy / ignore_zero: the reference flags.
 *   loss [1]; minmax [2][bq] (min_pos, max_pos); gradients of the loss: gq [bq][D], gpos [bq][P][D],
 *   gneg [bq][Ng][D], gother [bq][D].
 */
int lpd_metric_loss(const float* q, long long q_sb, const float* pos, long long pos_sb, long long pos_st,
                    const float* neg, long long neg_sb, long long neg_st, const float* other, long long other_sb,
                    int bq, int P, int Ng, int D, float m1, float m2, int use_min, int lazy, int ignore_zero, int quad,
                    float* loss, float* minmax, float* gq, float* gpos, float* gneg, float* gother, void* stream);

/* Backward of best_pos_distance (loss/pointnetvlad_loss.py:6-12) given the gradients of (min_pos, max_pos) [bq] each:
 * gq [bq][D], gpos [bq][P][D] (contiguous); q / pos addressed like lpd_metric_loss; P <= 64. */
int lpd_best_pos_bwd(const float* q, long long q_sb, const float* pos, long long pos_sb, long long pos_st, const float* gmin,
                     const float* gmax, int bq, int P, int D, float* gq, float* gpos, void* stream);

/*
 * Descriptor retrieval (evaluate.py:162-206: KDTree(database).query(query, k = 25) per query): the k nearest database
 * descriptors of every query by squared Euclidean distance, ascending, ties -> lower index.
 *   S [nq][ndb] = Q D^T (row-major, from lpd_gemm), Q [nq][ldq], D [ndb][ldd] the descriptors (for the norms),
 *   idx [nq][k] int32, dist [nq][k] squared distances, ws nq + ndb floats.
 */
int lpd_retrieval_topk(const float* S, const float* Q, int ldq, const float* D, int ldd, int nq, int ndb, int dim, int k,
                       int32_t* idx, float* dist, float* ws, void* stream);

/*
 * The recall evaluation of evaluate.py:33-93 (every (database run m, query run n) pair scored as in get_recall, evaluate.py:162-206)
 * in one launch over resident descriptor tables; the n_q x n_db score matrices are never stored.  Distances, ranking and ties are
 * those of lpd_retrieval_topk (exact f32-input MFMA dot products, fmaf-chain norms, max(|q|^2 + |d|^2 - 2 q.d, 0), ties -> lower index).
 *   Q [q_rows][ldq]: every query run concatenated, run n = rows q_off[n] .. q_off[n+1]; D [d_rows][ldd] likewise with d_off [rd+1]
 *   (q_off[0] = d_off[0] = 0; dim = 64, 128 or 256, ldq / ldd multiples of 4, 16-byte aligned tables: pad other descriptor sizes
 *   with zero channels, which change no result).  pairs [npairs][2] int32 = (m, n), npairs <= 65535.  Pair p's queries own the output rows
 *   out_off[p] .. out_off[p+1] (= the pair offsets, out_off[p+1] - out_off[p] = Nq of run n); max_qtiles = max over pairs of
 *   ceil(Nq / 128).  Truth lists as CSR: the list QUERY_SETS[n][i][m] of global query row g = q_off[n] + i is
 *   truth_idx[truth_off[g * rd + m] .. truth_off[g * rd + m + 1]) (row numbers inside run m).
 *   k <= 64; pair p ranks its k_p = min(k, Nd of run m) nearest rows.  Per (pair, query) row:
 *     first    int32: -1 = no truth in run m (not evaluated); k = no true neighbour within the k_p ranks; else the first rank that holds one
 *     one_pct  uint8: a true neighbour within the first min(max(round(Nd / 100), 1), k_p) ranks (round half to even, as Python's round)
 *     top1_sim fp32: dot product of the query with its rank-0 row (the top-1 similarity where first == 0)
 *     topk_idx int32 [k] (optional, NULL = not written): the ranked row numbers inside run m, -1 past k_p
 *   per pair: hist [npairs][k+1] (queries whose first hit is at rank r; column k = not found), n_eval [npairs] (evaluated queries),
 *   n_onepct [npairs] (one-percent hits) -- overwritten.  ws: q_rows + d_rows floats (the squared norms).  The caller guarantees that the
 *   offsets, pairs and truth_off index inside the tables (lpdnet_hip/ops.py recall_pairs checks them on the host).
 */
#define LPD_RECALL_KMAX 64
int lpd_recall_pairs(const float* Q, int ldq, const float* D, int ldd, int dim, const int32_t* q_off, const int32_t* d_off, int rd,
                     int q_rows, int d_rows, const int32_t* pairs, const int32_t* out_off, int npairs, int max_qtiles,
                     const int32_t* truth_off, const int32_t* truth_idx, int k, int32_t* first, uint8_t* one_pct, float* top1_sim,
                     int32_t* topk_idx, int32_t* hist, int32_t* n_eval, int32_t* n_onepct, float* ws, void* stream);

/*
 * Batched hard-negative selection (util/data.py:103-115, called for every item of the second training phase with 4000 sampled
 * negatives: a KDTree per query there): for query b, among the rows cand[b][0..nc) of the latent-vector table, the k nearest to
 * Q[b] by squared Euclidean distance, nearest first, as POSITIONS into cand[b] (ties -> lower position); dist [bq][k].
 *   table [n_items][ldt] (the descriptors of the whole training set, kept on the device), Q [bq][ldq], cand [bq][nc] int32.
 */
int lpd_hard_negatives(const float* table, long long ldt, const float* Q, long long ldq, const int32_t* cand, int bq, int nc, int dim,
                       int k, int32_t* pos, float* dist, void* stream);

/* float64 -> float32, n elements (submap files are float64, loading_pointclouds.py:26-35; evaluate.py:115 `.float()`). */
int lpd_f64_to_f32(const double* in, float* out, long long n, void* stream);

/* Per-cloud Morton (Z-order) reordering of the input points: out[b][r] = xyz[b][perm[b][r]].  The descriptor is
 * invariant to point order; sorting makes the neighbour gathers of the aggregation kernels cache-local.
 * xyz/out [B][N][3] (out != xyz), perm [B][N] int32 or NULL.  N <= 16384. */
int lpd_morton_sort(const float* xyz, float* out, int32_t* perm, int B, int N, void* stream);
/* Default path (the head of the LPD-Net eval forward): the same sort, which also leaves what the xyz search wants in its workspace
 * knn_ws (lpd_knn_workspace_floats(B, 3, N, k) floats, laid out by lpd_knn_pm_layout(B, 3, N, k, ...)): squared norms, the packed
 * operand image and the statistics of the 32-point tiles of the SORTED cloud, bit for bit what lpd_knn_pm on the sorted rows writes
 * there in its prep and tile-statistics launches.  lpd_knn_pm(NULL, 3, B, 3, N, k, idx, knn_ws, LPD_KNN_PM_PREPARED, stream) then
 * builds the graph without those launches.  lpd_morton_sort_knn_applies(N, k): N % 32 == 0, 64 <= N <= 16384 and the best-first
 * search on these sizes (LPD_DEBUG=sort-knn=0: never); LPD_ERR_UNSUPPORTED elsewhere. */
int lpd_morton_sort_knn_applies(int N, int k);
int lpd_morton_sort_knn(const float* xyz, float* out, int32_t* perm, int B, int N, int k, float* knn_ws, void* stream);

/*
 * Local point-distribution features from sorted neighbour lists (csrc/lpd_feat.hip): the handcrafted per-point columns that the
 * use_mFea trunks take behind xyz (reference lpdnet_model.py:183-186,215-224; the reference reads them from an offline step).
 *   xyz   [B*N][ldx] point-major, three coordinates used
 *   idx   [B][N][K] int32, local to the cloud, nearest first (lpd_knn_pm's output; any list is legal -- an index outside the cloud
 *         is read as the cloud's last point)
 *   cand  HOST array of ncand <= 16 strictly ascending neighbourhood sizes, 4 <= cand[i] <= K, read at call time and handed to the
 *         kernel by value; NULL / ncand == 0: one fixed size k = K.  With candidates the size with the smallest eigenentropy is
 *         used (ties: the smaller size) and ALL columns are taken at that size; the list is walked once, not once per candidate.
 *   sel   bit mask over the ten columns below; the selected ones are written in ascending column order to
 *         out[m*ldo + (copy_xyz ? 3 : 0) + j]; copy_xyz = 1 also writes the point's coordinates to the first three entries of the row
 *         (five columns, ldo = 8: the [B*N, 8] input rows of a use_mFea trunk from one launch).  Entries of a row behind the
 *         written ones are left untouched.
 *   kopt  [B*N] int32 or NULL: the neighbourhood size used for each point
 * For point i, list n_0 .. n_{K-1} and size k, with d_j = x_{n_j} - x_i over the first k entries (moments are accumulated on d_j,
 * centred on the query point): mu = mean d_j, S = mean d_j d_j^T - mu mu^T, l1 >= l2 >= l3 the eigenvalues of S clamped at 0
 * (six cyclic Jacobi sweeps in fp32), n the unit eigenvector of l3, s = l1 + l2 + l3, e_i = l_i / s.
 *   0 change of curvature e3         1 omnivariance cbrt(e1 e2 e3)       2 linearity (l1 - l2) / l1
 *   3 eigenentropy -sum e_i ln e_i   4 verticality |n_z|                 5 2-D scattering S_xx + S_yy
 *   6 2-D linearity: smaller / larger eigenvalue of the xy block of S    7 height range max d_j.z - min d_j.z
 *   8 height variance S_zz           9 density k / ((4/3) pi r^3), r = |d_{k-1}|
 * s == 0: columns 0-4 are 0; l1 == 0: 2 is 0; larger 2-D eigenvalue 0: 6 is 0; r == 0: 9 is 0.
 * Supported: 4 <= K <= 64, K <= N.  Clouds of N <= 4096 points are staged in LDS, larger ones read their neighbours through L2:
 * same bits either way.
 */
int lpd_local_features(const float* xyz, int ldx, const int32_t* idx, int B, int N, int K, const int32_t* cand, int ncand, unsigned sel,
                       int copy_xyz, float* out, int ldo, int32_t* kopt, void* stream);

/*
 * Submaps from raw scans (csrc/lpd_submap.hip): a ragged batch of B clouds of any length becomes [B][N][3] model input in one launch --
 * a voxel-grid average whose cell size is searched so that the number of occupied cells lands just under N, filled up to exactly N
 * with raw points, shifted to zero mean and scaled into [-1, 1].  The reference has no counterpart (its submaps come from an offline
 * preprocessing step that is not part of it); this comment is the specification.
 *   points   [rows][ld] fp32, ld >= 3, three coordinates used; finite
 *   offsets  DEVICE int32 [B+1], ascending: cloud b is rows offsets[b] .. offsets[b+1]-1; 1 <= length <= 2^20.  A cloud whose offsets
 *            break this (negative, empty, longer) is not read: its rows, counts and xform are 0 and its info is (-1, 0, 0, 0).
 *   out      [B][N][3]     info [B][4] int32 = (j*, M, n, 0)     xform [B][4] = (mean_x, mean_y, mean_z, r)
 *   counts   [B][N] int32 or NULL: points per cell on rows 0 .. M-1 (a density weight), 0 on the fill rows (their marker)
 * For one cloud of n points x_i and the target N, 128 <= N <= 4096; fp32 arithmetic, every operation rounded once (no contraction),
 * unless stated otherwise:
 *  1 Box.     mn_c = min_i x_ic,  E = max_c (max_i x_ic - mn_c).
 *  2 Ladder.  R_j = 1024 * 2^(-j/16) cells per E, j = 0 .. 127: the fp32 literal of 2^(-(j mod 16)/16) times 1024 times
 *             2^(-(j div 16)) (both exact).  s_j = R_j / E, one IEEE division per cloud and rung; E == 0: s_j = 0.
 *             Cell of a point: q_c = (uint32) min(max((x_c - mn_c) * s_j, 0), 1023); key = the 30-bit Morton interleave of q
 *             (x in bit 0, y in bit 1, z in bit 2 of each triple, as lpd_morton_sort).
 *  3 Search.  count(j) = number of distinct keys.  lo = -1, hi = 127; while hi - lo > 1: mid = (lo + hi) / 2; count(mid) <= N ?
 *             hi = mid : lo = mid.  j* = hi after 7 steps.  count is NOT monotone in j: j* is the outcome of this bisection, not a
 *             minimum.  Rung 127 has at most 5 cells per axis (125 <= N), so the search cannot fail: hence N >= 128.
 *  4 Cells.   The M = count(j*) cells in ascending key order are rows 0 .. M-1.  u_c = rint((x_c - mn_c) * f), f = 2^20 / E (0 if
 *             E == 0), half to even; S_c = sum of u_c in unsigned 64-bit integers, m = number of points of the cell;
 *             row_c = mn_c + (float)((double)S_c / (double)m) * (E * 2^-20).  Integer sums: exact in any order.
 *  5 Fill.    Rows M + p, p = 0 .. N-M-1, are raw points unchanged: x_i with i = ((2p + 1) * n) / (2 (N - M)), 64-bit floor division.
 *  6 Normalise (normalize = 1).  mean_c = the fp64 sum of the N rows in a fixed order, divided by N, rounded to fp32; d = row - mean;
 *             r = max |d| over rows and axes; out = d * (1.0f / r), all zeros if r == 0.  xform = (mean, r): row = out * r + mean.
 *             normalize = 0: the rows of 4 and 5 are written as they are and xform = (0, 0, 0, 1).
 * The result does not depend on thread order; rows 0 .. M-1, info and counts do not depend on the order of the raw points either
 * (the fill rows do, by definition).  No float atomics.  One 1024-thread workgroup per cloud; N > 4096: LPD_ERR_UNSUPPORTED.
 */
#define LPD_SUBMAP_MIN_N 128           /* rung 127 has at most 125 cells, so the search cannot fail for N >= 128 */
#define LPD_SUBMAP_MAX_N 4096
#define LPD_SUBMAP_MAX_POINTS 1048576  /* raw points per cloud: 2^20 points x 2^20 quantisation steps stay far inside 64 bits */
int lpd_make_submaps(const float* points, int ld, const int32_t* offsets, int B, int N, int normalize, float* out, int32_t* info,
                     float* xform, int32_t* counts, void* stream);

/*
 * Training tuples on the device (csrc/lpd_tuples.hip; arithmetic in csrc/lpd_tuple_math.h): what the reference's Dataset.__getitem__
 * does in Python per query (util/data.py:56-101 shuffles and set differences; loading_pointclouds.py:50-85 rotation and jitter) as two
 * launches over tables that stay on the device.
 *
 * lpd_sample_items: distinct items drawn uniformly from a union of item lists, or from its complement; one launch, R rows.
 *   T        number of items, 1 <= T <= 262144 (the membership bitmap and its scanned popcounts are 64 KiB of LDS at the limit)
 *   off/idx  CSR of n_lists lists over the items: list l = idx[off[l] .. off[l+1]), int32, nnz = entries of idx; duplicates and any
 *            order allowed.  off is ascending within [0, nnz]; whatever lies outside is clipped to it.
 *   lists    [R][L] list numbers of row r, -1 = unused slot, 0 <= L <= 64        extra [R][X] single items, -1 = unused, 0 <= X <= 64
 *   invert   0 or 1        m  samples per row, 1 <= m <= 4096        seed  64 bits        1 <= R <= 65535
 *   S_r = the union of the row's lists and extras; the pool is S_r (invert = 0) or [0, T) \ S_r (invert = 1); z_0 < ... < z_{c-1} its
 *   members in ascending order.  count[r] = c;  out[r][j] = z_{perm(j, c, seed, r)} for j < min(m, c),  -1 for c <= j < m.
 *   perm(., c, seed, r) is a bijection of [0, c) made of 32-bit integer operations only (a 4-round Feistel network with cycle walking);
 *   csrc/lpd_tuple_math.h is its definition.  A list number outside [0, n_lists) and an item outside [0, T) -- in lists, extra or
 *   idx -- is IGNORED and never used as an address.  No float arithmetic, no atomics on global memory: equal bits in every launch.
 *
 * lpd_gather_tuples: the model's input from the resident table.
 *   table [T][N][3] contiguous, items [B] int32 on the device, out [B][N][3] (not the table), 1 <= B <= 65535, 1 <= N <= 2^20
 *   rot   [B][2] = (cos, sin) of the angle of slot b, or NULL:  x' = x c + y s,  y' = -x s + y c,  z' = z  (the reference's pc @ R;
 *         two products and a sum, each rounded once)
 *   sigma, clip, seed: then out += delta,  delta_i = clamp(sigma z_i, -clip, clip),  z from Philox4x32-10 with counter
 *         (point n, slot b, 0, 0) and key (seed low word, seed high word) through Box-Muller (lpd_tuple_math.h).  sigma = 0: no jitter,
 *         Philox is never evaluated.  sigma >= 0, clip > 0.
 *   Without rot and with sigma = 0 the output rows are bit-copies of the table rows.  An item outside [0, T) gives a cloud of zeros
 *   (no jitter either) and is never read.  N % 4 == 0 with 16-byte aligned table / out: 16-byte accesses, one point per thread else.
 */
#define LPD_TUPLE_MAX_ITEMS 262144     /* T: the membership bitmap (32 KiB) and its scanned popcounts (32 KiB) live in LDS */
#define LPD_TUPLE_MAX_SAMPLES 4096     /* m */
#define LPD_TUPLE_MAX_LISTS 64         /* L and X */
#define LPD_TUPLE_MAX_ROWS 65535       /* R, and B of lpd_gather_tuples (one grid dimension) */
int lpd_sample_items(const int32_t* off, const int32_t* idx, int n_lists, int nnz, int T, const int32_t* lists, int L, const int32_t* extra,
                     int X, int R, int invert, int m, unsigned long long seed, int32_t* out, int32_t* count, void* stream);
int lpd_gather_tuples(const float* table, int T, int N, const int32_t* items, int B, const float* rot, float sigma, float clip,
                      unsigned long long seed, float* out, void* stream);

/*
 * Place lists from positions (csrc/lpd_places.hip; the predicate in csrc/lpd_places_math.h): which database items lie within a radius
 * of each query position, per database segment, as sorted CSR rows.  What the reference's generating_queries/ scripts make on the
 * host with sklearn's KDTree.query_radius over (northing, easting): generate_training_tuples_baseline.py:52-72 at r = 10 m (positives)
 * and r = 50 m (the non-negatives), generate_test_sets.py:99-109 at r = 25 m (the truth lists of the evaluation).
 *   qpos     [Q][2] float64 query positions         dpos  [D][2] float64 database positions; both 16-byte aligned
 *   seg_off  DEVICE int32 [S+1], rising from 0 to D: segment s (one database run; S = 1 for training) is the items
 *            seg_off[s] .. seg_off[s+1]-1.  Whatever lies outside [0, D] is clipped to it; nothing outside the table is read.
 *   r        the radius, finite, >= 0
 * Row g * S + s (query g, segment s) holds, in ascending order, the LOCAL indices j - seg_off[s] of the items j of segment s with
 *     dx = qpos[g][0] - dpos[j][0];   dy = qpos[g][1] - dpos[j][1];   (dx * dx) + (dy * dy) <= r * r
 * in float64, every operation rounded once, nothing contracted, r * r ONE product.  A NaN on either side is never a member (nor is
 * an infinite coordinate); (a - b)^2 == (b - a)^2 exactly, so membership is symmetric in the two positions.  Float64 is part of the
 * definition: at a UTM northing of 5.7e6 an fp32 ulp is 0.5 m.  On boundary points -- offsets (6, 8), (8, 6), (10, 0) at r = 10 -- the
 * rule includes the item, as KDTree.query_radius does.
 *   skip_seg   [Q] int32 or NULL: skip_seg[g] == s makes row (g, s) empty (generate_test_sets.py:102 `if i == j: continue`); -1 = none
 *   self_item  [Q] int32 or NULL: the GLOBAL database index self_item[g] is left out of the rows of query g (np.setdiff1d(ind_nn[i],
 *              [i]) of generate_training_tuples_baseline.py:59); -1 = none
 * lpd_radius_count writes counts [Q * S] int32, the row lengths.  lpd_radius_fill takes row_off [Q * S + 1], the exclusive scan of
 * the counts (the caller's: torch.cumsum in lpdnet_hip/ops.py), and writes idx [nnz], nnz = row_off[Q * S]; an entry whose place
 * falls outside [0, nnz) -- a row_off that is not that scan -- is dropped, not written.  Both calls run one kernel on the same
 * predicate, so the counts and the fill agree; the order within a row comes from the kernel's construction (candidates in
 * ascending order, __ballot and a popcount of the lanes below), not from a sort.  No atomics: the same bits in every launch.
 * Limits: 1 <= S <= 4096, 0 <= Q, D <= 2^22, Q * S < 2^31.  Q == 0 launches nothing.
 */
#define LPD_PLACES_MAX_ITEMS 4194304   /* Q and D: 2^22 */
#define LPD_PLACES_MAX_SEGMENTS 4096   /* S (one grid dimension) */
#define LPD_PLACES_CHUNK 1024          /* candidate positions staged in LDS at a time (16 KiB) */
int lpd_radius_count(const double* qpos, int Q, const double* dpos, int D, const int32_t* seg_off, int S, double r, const int32_t* skip_seg,
                     const int32_t* self_item, int32_t* counts, void* stream);
int lpd_radius_fill(const double* qpos, int Q, const double* dpos, int D, const int32_t* seg_off, int S, double r, const int32_t* skip_seg,
                    const int32_t* self_item, const int32_t* row_off, int32_t* idx, int nnz, void* stream);

/*
 * Road removal and range crop for raw scans (csrc/lpd_clean.hip; arithmetic in csrc/lpd_clean_math.h): the step in front of
 * lpd_make_submaps.  The reference's models are trained on submaps "preprocessed with the road removed" by an offline step that is not
 * part of it; this comment is the specification, and lpd_clean_math.h settles every detail it leaves open.  A deterministic road-plane
 * estimator (scored random triples, one least-squares round), a crop, and a stable ragged compaction; no read-back.
 *   points   [rows][ld] fp32, ld >= 3, three coordinates used; NaN and inf allowed (such rows are not live)
 *   offsets  DEVICE int32 [B+1]: scan b is rows offsets[b] .. offsets[b+1]-1.  A scan whose offsets are negative, empty, longer than
 *            max_len (the caller's bound on the longest scan, 1 .. 2^20; it sizes the grid) or end behind `rows` is NOT READ: it keeps
 *            0 rows, its plane is 0 and its info is (-1, -1, 0, 0).
 *   prm      LpdCleanParams in HOST memory (read by the call).  0 <= r_min <= r_max <= 512 m; 0 <= H <= 1024; tau, min_det, max_slope
 *            finite and >= 0; clearance finite; the z limits may be +-inf but not NaN; min_inliers >= 0; refine 0 or 1.
 * For one scan of n rows, fp32, every operation rounded once, no contraction, IEEE division, every comparison false on NaN:
 *  1 Live.     x, y, z finite;  r_min*r_min <= (x*x) + (y*y) <= r_max*r_max (each square on the outside ONE product);  z_lo <= z <= z_hi.
 *  2 Hypotheses h = 0 .. H-1.  (r0, r1, r2, _) = lpd_philox4x32_10(h, b, 0, 0, seed_lo, seed_hi);  rows i_j = ((uint64) r_j * n) >> 32.
 *              Valid iff the three rows are live and seed_z_lo <= z <= seed_z_hi, and with u = p1 - p0, v = p2 - p0,
 *              det = (u_x*v_y) - (u_y*v_x):  |det| >= min_det,  a = ((u_z*v_y) - (v_z*u_y)) / det,  b = ((u_x*v_z) - (v_x*u_z)) / det,
 *              c = z0 - ((a*x0) + (b*y0)),  (a*a) + (b*b) <= max_slope*max_slope,  c finite.  The plane is z = a x + b y + c.
 *  3 Score.    e_i = z_i - (((a*x_i) + (b*y_i)) + c);  S(h) = number of live rows with fabsf(e_i) <= tau.  h* = the valid h with the
 *              largest S, ties to the lowest h.  No valid h, or S(h*) < min_inliers: "no road" -- the road rule removes nothing, the
 *              plane is 0, info = (n_live, -1, the largest S of a valid h or 0, 0).  H = 0: no road step at all, crop only.
 *  4 Refine (refine = 1, one round).  o = p0 of h*.  Over the inliers of h*: X = (int) rintf((x - o_x) * 1024.0f), clamped to +-2^20,
 *              Y and Z alike; the nine sums m, SX, SY, SZ, SXX, SXY, SYY, SXZ, SYZ in 64-bit integers (exact in any order); then in
 *              float64, in the order written in lpd_clean_solve: cxx = SXX - SX*SX/m ..., D = cxx*cyy - cxy*cxy,
 *              a' = (cxz*cyy - cyz*cxy) / D, b' = (cyz*cxx - cxz*cxy) / D, c' = (SZ - a'*SX - b'*SY) / m,
 *              c = (float)(o_z + c'/1024 - a'*o_x - b'*o_y); a, b rounded to fp32.  The plane of h* is kept when m < 3, D is not
 *              positive and finite, or the refined slope breaks max_slope.
 *  5 Remove.   A live row is removed iff z - (((a*x) + (b*y)) + c) <= clearance: the road and everything under it.  The rows that
 *              are kept stay in their order (a stable compaction).
 * lpd_road_planes writes plane [B][4] = (a, b, c, 0) and info [B][4] int32 = (n_live, h* or -1, S(h*), inliers of the final plane);
 * ws = lpd_road_planes_workspace_bytes(B, H) bytes, 16-byte aligned, the caller's, no state between calls.  The plane depends on the
 * order of the rows (the triples are drawn by row number); for a given plane, which rows are kept does not.
 * lpd_clean_count writes counts [B * chunks] int32, chunks = ceil(max_len / LPD_CLEAN_CHUNK): the rows kept in each 1024-row chunk of
 * each scan.  lpd_clean_fill takes block_off [B * chunks + 1], the exclusive scan of the counts (the caller's: torch.cumsum in
 * lpdnet_hip/ops.py), and writes out [rows][3] (the kept rows of scan 0, then scan 1, ...: bit-copies), out_offsets [B+1] on the DEVICE
 * (out_offsets[b] = block_off[b * chunks], out_offsets[B] = block_off[B * chunks]) and, when not NULL, mask [rows] uint8: 1 = kept,
 * 0 = dropped, for the rows of scans that are read (the others are left as they are).  A place outside [0, rows) -- a block_off that
 * is not that scan -- is dropped, not written.  plane and info NULL (both): crop only.  Both calls run one kernel on the same
 * predicate.  Integer atomics only, no float atomics: the same bits in every launch.  1 <= B <= 65535.
 */
#define LPD_CLEAN_CHUNK 1024           /* rows of one workgroup */
#define LPD_CLEAN_MAX_H 1024           /* hypotheses per scan */
typedef struct LpdCleanParams {
    float r_min, r_max, z_lo, z_hi, seed_z_lo, seed_z_hi, tau, min_det, max_slope, clearance;
    int32_t H, min_inliers, refine;
    uint32_t seed_lo, seed_hi;      /* the two words of the 64-bit seed: the Philox key */
    int32_t reserved;               /* 0 */
} LpdCleanParams;
long long lpd_road_planes_workspace_bytes(int B, int H);
int lpd_road_planes(const float* points, int ld, int rows, const int32_t* offsets, int B, int max_len, const LpdCleanParams* prm,
                    float* plane, int32_t* info, void* ws, void* stream);
int lpd_clean_count(const float* points, int ld, int rows, const int32_t* offsets, int B, int max_len, const LpdCleanParams* prm,
                    const float* plane, const int32_t* info, int32_t* counts, void* stream);
int lpd_clean_fill(const float* points, int ld, int rows, const int32_t* offsets, int B, int max_len, const LpdCleanParams* prm,
                   const float* plane, const int32_t* info, const int32_t* block_off, float* out, int32_t* out_offsets,
                   unsigned char* mask, void* stream);

/*
 * Submaps from a drive (csrc/lpd_drive.hip; arithmetic in csrc/lpd_drive_math.h): posed scans cut by distance travelled into windows,
 * each window brought into one frame.  The reference's .bin submaps and its pointcloud_locations_20m_10overlap.csv (20 m windows every
 * 10 m for training, every 20 m for testing) come from an offline step that is not part of it; this comment is the specification, and
 * lpd_drive_math.h settles every detail it leaves open.  The step in front of lpd_clean_* and lpd_make_submaps; no read-back.
 *   points   [rows][ld] fp32, ld >= 3, three coordinates used, each scan in its own sensor frame
 *   offsets  DEVICE int32 [S+1]: scan i is rows offsets[i] .. offsets[i+1]-1 (a scan may have no rows)
 *   poses    [S][12] float64 on the device: the top three rows of the homogeneous sensor-to-world matrix, row-major (R | t) -- a line of
 *            a KITTI poses.txt.  Float64 is part of the definition: at a UTM northing of 5.7e6 an fp32 ulp is 0.5 m.
 * Float64 and fp32 alike: every operation rounded once, nothing contracted; every dot product is ((a0*b0) + (a1*b1)) + (a2*b2).
 *  1 Steps.    dl_0 = 0;  d = t_i - t_{i-1},  dl_i = sqrt(((dx*dx) + (dy*dy)) + (dz*dz)) in float64 with the correctly rounded square
 *              root;  q_i = (int64) rint(dl_i * 65536.0) clamped to [0, 2^36];  a dl_i that is not finite gives q_i = 0.  Distances are
 *              integers in units of 2^-16 m from here on: their sums are exact in any order.
 *  2 Distance. D_i = q_0 + ... + q_i (the caller's: torch.cumsum on int64 in lpdnet_hip/ops.py).
 *  3 Windows.  L = rint(length * 65536), T = rint(stride * 65536) (the caller's, 1 <= L, T <= 2^40).  lower_bound(D, v) = the first i
 *              with D_i >= v, S when there is none.  Window w is the scans first_w = lower_bound(D, w*T) .. end_w - 1 with
 *              end_w = lower_bound(D, w*T + L): a scan with D_i == w*T + L belongs to the next range.  Its reference scan is
 *              ref_w = min(lower_bound(D, w*T + L/2), end_w - 1), L/2 the integer quotient.  first_w == end_w is an EMPTY window (a
 *              single step longer than L): ref = -1, no rows, position 0.  The windows of the drive are the w with w*T + L <= D_{S-1};
 *              a window behind them is written as (S, S, -1, 0), empty.  A scan lies in at most ceil(L / T) windows.
 *  4 Plan.     plan [W][4] int32 = (first, end, ref, rows), rows = offsets[end] - offsets[first]: a window's rows are ONE contiguous
 *              range of the input rows.  position [W][3] float64 = t_ref, bit-copies.  The output offsets are the exclusive scan of
 *              `rows` (the caller's torch.cumsum again).
 *  5 Relative pose of scan i in window w, float64:  frame = 1 (the reference scan's own frame)  M = R_ref^T R_i,
 *              u = R_ref^T (t_i - t_ref);  frame = 0 (world axes moved to the reference scan's position)  M = R_i, u = t_i - t_ref.
 *              The difference is taken first (three subtractions); the twelve numbers are rounded to fp32 once.
 *  6 Rows.     out_c = (((M_c0*x) + (M_c1*y)) + (M_c2*z)) + u_c in fp32.  A NaN or inf coordinate passes through as the arithmetic
 *              gives it (the cleaning behind drops it); the scan of a row is the last i with offsets[i] <= row.
 * lpd_drive_steps writes q [S] int64.  lpd_drive_plan writes plan and position for the windows w0 .. w0+W-1 (a long drive is planned in
 * batches; w0 >= 0, w0 + W <= 2^22).  lpd_drive_rows writes out [out_off[W]][3]: the rows of window 0 of the call at out_off[0], ...;
 * out_off DEVICE int32 [W+1]; max_len (1 .. 2^20) is the caller's bound on the longest window and sizes the grid.  A window is NOT
 * WRITTEN when its rows exceed max_len, when its plan line is not one (not 0 <= first <= ref < end <= S, rows != offsets[end] -
 * offsets[first], input rows outside [0, rows)) or when out_off[w+1] - out_off[w] != rows or out_off[w] < 0.  Nothing outside [0, S) of
 * the poses, [0, S] of the offsets and [0, rows) of the points is ever read, whatever the tables hold; no row is used as an address.
 * No atomics: the same bits in every launch.  Limits: 1 <= S <= 2^22, 1 <= W <= 65535 per call, fewer than 2^31 output rows.
 */
#define LPD_DRIVE_MAX_SCANS 4194304        /* S: 2^22 */
#define LPD_DRIVE_MAX_WINDOWS 65535        /* W of one call */
#define LPD_DRIVE_MAX_WINDOW_NO 4194304    /* w0 + W: with L, T <= 2^40 and D <= 2^22 * 2^36 every sum of the plan stays under 2^63 */
#define LPD_DRIVE_MAX_UNITS 1099511627776  /* L and T, in units of 2^-16 m: 2^40 */
int lpd_drive_steps(const double* poses, int S, long long* q, void* stream);
int lpd_drive_plan(const long long* D, int S, const int32_t* offsets, const double* poses, long long L, long long T, long long w0, int W,
                   int32_t* plan, double* position, void* stream);
int lpd_drive_rows(const float* points, int ld, int rows, const int32_t* offsets, const double* poses, int S, const int32_t* plan, int W,
                   const int32_t* out_off, int frame, int max_len, float* out, void* stream);

/*
 * Geometric verification of retrieved places (csrc/lpd_align.hip; arithmetic in csrc/lpd_align_math.h): correlative scan matching
 * (Olson, "Real-time correlative scan matching", ICRA 2009) of (query, candidate) submap pairs.  Both clouds are rasterised into
 * bird's-eye occupancy bitmaps with a few height layers; yaw is searched over a caller-made table and a window of cell shifts is
 * searched exhaustively; the score is a popcount of ANDed bitmaps.  The step behind lpd_recall_pairs' topk_idx / lpd_retrieval_topk:
 * which candidate is geometrically the same place, and the relative pose to it.  This comment is the specification, and
 * lpd_align_math.h settles every detail it leaves open.  Integer-only once the cells are assigned; no initial guess; no read-back.
 *   A        [TA][N][3] fp32; may be the same table as B.  B [TB][N][3] fp32.  1 <= N <= 16384.  NaN and inf allowed (no bit is set).
 *   scaleA   [TA] fp32 metres per unit (Submaps.scale), or NULL for 1.0f; scaleB [TB] alike
 *   pairs    [P][2] int32 = (row of A, row of B), 1 <= P <= 2^20.  A pair that names a row outside its table is NEVER READ: its best is
 *            (-1, 0, 0, 0, 0, 0, 0, 0) and its yaw_scores are 0.
 *   rot      [R][2] fp32 = (cos, sin), the CALLER's table (made once on the host): no trigonometric function is evaluated on the device.
 *            Pair p uses the entries rot[(first[p] + h) mod R] (the non-negative remainder), h = 0 .. H-1; first [P] int32, or NULL for 0.
 *            1 <= H <= R <= 8192, H <= 1024.  The integer indirection lets a coarse-to-fine chain stay on the device, bit-exact.
 *   t0       [P][2] fp32 metres: a pre-translation of A, or NULL
 * fp32, every operation rounded once, no contraction, every comparison false on NaN.  For a point (x, y, z) of cloud i and (c, s):
 *  1 Scale.    p = (x*sc, y*sc, z*sc), sc = scale[i] or 1.0f.
 *  2 Rotate (A only).  xr = (px*c) - (py*s),  yr = (px*s) + (py*c);  then xr = xr + t0x, yr = yr + t0y when t0 is given.  B: xr = px,
 *              yr = py.
 *  3 Cell.     fx = floorf(xr * inv_cell) + 64.0f, valid iff fx >= 0.0f && fx < 128.0f, ix = (int) fx only after that test; iy alike;
 *              fz = floorf((pz - z0) * inv_zcell), valid iff 0 <= fz < layers.  A point with any invalid index, or any non-finite
 *              coordinate, sets no bit.
 *  4 Bitmap.   occ[layer][iy] is a 128-bit row, bit ix set.  The grid is fixed at 128 x 128 cells; layers 1 .. 4.
 *  5 Score.    score(h, dy, dx) = sum over layers and rows iy of popcount(shift(occA_h[l][iy], dx) & occB[l][iy + dy]);  shift moves
 *              bit ix to ix + dx, bits that leave [0, 128) are dropped; rows with iy + dy outside [0, 128) are dropped.
 *              dy, dx in [-S, S], 0 <= S <= 16.
 *  6 Winner.   The largest score; ties to the smallest (h, dy, dx) in lexicographic order, dy and dx counted from -S.
 *  7 Meaning.  p_B ~ R(yaw_h) p_A + t0 + (dx, dy) * cell, with cell = 1 / inv_cell.
 * best [P][8] int32 = (h, dy, dx, score, nA, nB, 1, 0): nA = the occupied cells of A at the winning yaw, nB = the occupied cells of B.
 * yaw_scores [P][H] int32, or NULL: the maximum over the shifts for every hypothesis.  inv_cell, inv_zcell finite and > 0, z0 finite.
 * ws = lpd_align_workspace_bytes(P, H) bytes (may be 0: then ws may be NULL), 16-byte aligned, the caller's, one per call in flight, no
 * state between calls: for a small P the hypotheses of a pair are spread over several workgroups, whose packed (score, inverted
 * candidate number) keys are combined by an integer maximum in a fixed order.  No float atomics; integer LDS atomics only: the same
 * bits in every launch and in any thread order.
 */
#define LPD_ALIGN_GRID 128             /* cells per side; a row of the bitmap is 128 bits = four 32-bit words, bit ix in word ix >> 5 */
#define LPD_ALIGN_MAX_LAYERS 4
#define LPD_ALIGN_MAX_S 16             /* |dy|, |dx| <= S <= 16: a shift never crosses a whole word */
#define LPD_ALIGN_MAX_H 1024           /* hypotheses per pair */
#define LPD_ALIGN_MAX_R 8192           /* entries of the (cos, sin) table */
#define LPD_ALIGN_MAX_POINTS 16384     /* points per cloud: a score and a cell count fit 15 bits */
#define LPD_ALIGN_MAX_PAIRS 1048576
long long lpd_align_workspace_bytes(int P, int H);
int lpd_align_pairs(const float* A, int TA, const float* scaleA, const float* B, int TB, const float* scaleB, int N,
                    const int32_t* pairs, int P, const float* rot, int R, const int32_t* first, int H, const float* t0,
                    float inv_cell, int S, float z0, float inv_zcell, int layers,
                    int32_t* best, int32_t* yaw_scores, void* ws, void* stream);

/*
 * Refinement of a verified match to a full 6-DoF pose (csrc/lpd_icp.hip; arithmetic in csrc/lpd_icp_math.h): trimmed point-to-plane
 * ICP (Chen and Medioni 1992; the linearised form of Low 2004) of (query, candidate) pairs, started from the yaw and shift of
 * lpd_align_pairs, and the normals it needs.  The step behind lpd_align_pairs: roll, pitch and z, and a measure of how well the
 * clouds fit.  This comment is the specification, and lpd_icp_math.h settles every detail it leaves open.  fp32 unless stated, every
 * operation rounded once, nothing contracted, every comparison false on NaN, dot products ((a0*b0) + (a1*b1)) + (a2*b2).
 *
 * lpd_point_normals: unit normals of a cloud's points from its kNN lists.
 *   xyz [B*N][ldx], idx [B][N][K] as for lpd_local_features, its rule for an index outside the cloud included (the cloud's last point
 *   is read instead); 4 <= K <= 64, K <= N.  The moments and the covariance are lpd_feat_add / lpd_feat_cov over the K entries, centred
 *   on the query point; the eigenvectors come from lpd_feat_math.h's six Jacobi sweeps carrying all three rows of V.
 *   normals [B*N][3] = the unit eigenvector of the smallest eigenvalue, normalised once more in fp32; its sign is what the sweeps give.
 *   (0, 0, 0) when the neighbourhood has no extent (l1 == 0) or a moment is not finite: "this point takes no part" downstream.
 *   flatness [B*N] or NULL = l3 / l2, 0 where l2 == 0 or the normal is 0.  Clouds of N <= 4096 are staged in LDS, larger ones are read
 *   through L2 (LPD_DEBUG=normals-l2 sends every cloud that way): the same bits.
 *
 * lpd_icp_pairs.
 *   A, B, scaleA, scaleB, pairs: exactly those of lpd_align_pairs; a pair that names a row outside its table is NEVER READ.
 *   1 <= N <= 16384, 1 <= P <= 2^20.  normalsB [TB][N][3].
 *   pose     [P][12] float64, IN and OUT: the top three rows of the homogeneous matrix, row-major (R | t), the layout of lpd_drive_*'s
 *            poses: p_B ~ R p_A + t in the clouds' scaled (metric, centred) frames.
 *   dmax     HOST array of iters + 1 fp32 distances, read by the call; every entry finite, > 0 and <= 16.  0 <= iters <= 64.
 *            6 <= min_inliers.
 * iters + 1 passes; pass s is computed at the pose that pass s - 1 left:
 *  1 Transform.  (M, u) = the pose rounded to fp32 once; a = (x*sc, y*sc, z*sc); p_c = (((M_c0*a_x) + (M_c1*a_y)) + (M_c2*a_z)) + u_c.
 *              A point with a non-finite p or any |p_c| > 512 has no correspondence.
 *  2 Correspondence.  q_j = B's point j scaled; d = q_j - p, d2_j = ((dx*dx) + (dy*dy)) + (dz*dz); j* = the j with the smallest d2,
 *              ties to the lowest j, a non-finite q_j never wins.  The correspondence is j* iff d2_{j*} <= dmax_s * dmax_s (one
 *              product) and normalsB[j*] is not (0, 0, 0); otherwise there is none.  Only this outcome is specified.
 *  3 Sums.     e = q - p, r = ((e_x*n_x) + (e_y*n_y)) + (e_z*n_z), c = p x n (each component (p_y*n_z) - (p_z*n_y) and so on),
 *              J = (c, n); Ji = (int64) rint(J * 1024) clamped to +-2^20, half to even, ri alike.  32 int64 per (pass, pair):
 *              [0] m, [1..21] sum Ji_a Ji_b for a <= b (row-major), [22..27] sum Ji_a ri, [28] sum ri ri, [29..31] 0.  Exact in any order.
 *  4 Step (passes 0 .. iters-1), float64, in the order written in lpd_icp_solve: H x = g by an unpivoted LDL^T.  Refused -- the pose
 *              stays bit for bit -- when m < min_inliers or a pivot is not positive and finite (or x or the new pose is not finite).
 *              Otherwise w = x[0..2], dt = x[3..5], dR = the rotation of the unit quaternion (1, w/2) / |(1, w/2)| (+, -, *, /, sqrt
 *              only), R <- dR R, t <- dR t + dt.
 * sums [iters+1][P][32] int64 receives every pass's sums; nn [P][N] int32, or NULL: the LAST pass's correspondence of every point of
 * A, or -1; info [P][4] int32 = (1 for a valid pair else -1, steps applied, steps refused, correspondences of the last pass).  An
 * invalid pair's pose is left as it is, its sums are 0 and its nn row -1.  ws = lpd_icp_workspace_bytes(P, N, iters) bytes (0: bad
 * dims), 16-byte aligned, the caller's, one per call in flight, no state between calls.  Integer atomics only: the same bits in every
 * launch.  Every call only enqueues.
 */
#define LPD_ICP_MAX_POINTS 16384       /* points per cloud: 2^14 terms of at most 2^40 in a sum */
#define LPD_ICP_MAX_PAIRS 1048576
#define LPD_ICP_MAX_ITERS 64
#define LPD_ICP_MIN_INLIERS 6          /* the least min_inliers: six unknowns */
#define LPD_ICP_SUMS 32                /* int64 entries of a (pass, pair): 29 used, 29..31 are 0 */
long long lpd_icp_workspace_bytes(int P, int N, int iters);
int lpd_point_normals(const float* xyz, int ldx, const int32_t* idx, int B, int N, int K, float* normals, float* flatness, void* stream);
int lpd_icp_pairs(const float* A, int TA, const float* scaleA, const float* B, int TB, const float* scaleB, const float* normalsB, int N,
                  const int32_t* pairs, int P, const float* dmax, int iters, int min_inliers, double* pose, int32_t* info,
                  long long* sums, int32_t* nn, void* ws, void* stream);

/*
 * Sequence-consistent place retrieval (csrc/lpd_seqmatch.hip; arithmetic in csrc/lpd_seq_math.h): every retrieved candidate of a
 * query is scored along the drive -- a short sequence of consecutive query rows against a line of consecutive database rows, at a
 * few velocities and shifts (Milford and Wyeth, "SeqSLAM", ICRA 2012; on these descriptors Liu et al., "SeqLPD", IROS 2019) -- and
 * the candidates are re-ranked by that score.  The step between lpd_retrieval_topk / lpd_recall_pairs' topk_idx and lpd_align_pairs.
 * This comment is the specification, and lpd_seq_math.h settles every detail it leaves open.  Integers only behind the quantisation.
 *   Q [nq][ldq], D [nd][ldd]  fp32 descriptor tables in drive order; dim 64, 128 or 256; ldq, ldd multiples of 4, tables 16-byte
 *            aligned (as for lpd_recall_pairs); Q and D may be the same memory.  NaN and inf allowed.
 *   q_off [SQ+1], d_off [SD+1]  int32 run offsets rising from 0 to nq / nd.  The run of a row x is found by a lower-bound search; a
 *            sequence never crosses a run boundary.  Only compared, never used as an address.
 *   cand     [nq][K] int32 database rows, 1 <= K <= 64.  An entry < 0 or >= nd is SKIPPED: none of its rows are read.
 *   steps    [V][L] int32, L = 2h + 1, 1 <= h <= 15, the CALLER's table (made once on the host from the velocities): steps[v][t+h] is
 *            the database offset of term t, steps[v][h] == 0.  The device never sees a velocity as a float.
 *   S        shifts s = -S .. S of the candidate row, 0 <= S <= 15; the caller keeps max|steps| + S <= 15.  V (2S+1) <= 1024.
 *   min_terms  1 .. L.
 * Distance of query row a and database row b, the arithmetic of lpd_retrieval_topk: squared norms by an fmaf chain in channel order,
 * q.d on the exact f32-input MFMA (the k-ordered fmaf chain), x = (qn + dn) - (2.0f * dot).  A NaN x makes the term "not counted";
 * otherwise d2 = fmaxf(x, 0.0f) and dq = (int) rintf(fminf(d2, 16.0f) * 16384.0f): the quantum is 2^-14, dq <= 2^18.
 * Candidate (i, r) has the centre row j = cand[i][r].  Hypothesis e = v (2S+1) + (s + S).  Term t = -h .. h pairs query row a = i + t
 * with database row b = j + s + steps[v][t+h]; it is counted iff a lies in the run of i, b lies in the run of j + s, and x is not NaN
 * (and b lies in j-15 .. j+15, which the caller's table guarantees).  sum_e = the sum of the counted dq (< 2^23), n_e their number.
 * The hypothesis is valid iff 0 <= j+s < nd, j+s lies in the run of j, and n_e >= min_terms.  e1 is better than e2 iff
 * (int64) sum1 * n2 < (int64) sum2 * n1; equal means go to the lower e: a total order, any reduction order gives the same winner.
 *   best     [nq][K][4] int32 = (e, sum, n, j + s) of the best valid hypothesis; (-1, 0, 0, -1) for a skipped candidate or one
 *            without a valid hypothesis.
 *   order    [nq][K] int32: a permutation of 0 .. K-1 per query; valid candidates first by the same comparison of means (ties to
 *            the lower r), then the others in retrieval order.
 *   block    [nq][K][32][32] int32, or NULL: entry [t+h][b'] = dq of query row i + t, t = -h .. h, against database row j - 15 + b',
 *            whatever runs the rows lie in; -1 where either row is outside its table or x is NaN, in the rows t + h > 2h, in row 31
 *            and column 31, and everywhere for a skipped candidate.
 *   ws       nq + nd floats, the caller's: the squared norms.  No state between calls.
 * No atomics of any kind: the same bits in every launch.  Nothing outside the tables is read whatever cand, steps and the offsets
 * hold.  The call only enqueues.
 */
#define LPD_SEQ_BAND 15
#define LPD_SEQ_QBITS 14
#define LPD_SEQ_KMAX 64
#define LPD_SEQ_MAX_HYP 1024
int lpd_seq_match(const float* Q, int ldq, int nq, const int32_t* q_off, int SQ,
                  const float* D, int ldd, int nd, const int32_t* d_off, int SD, int dim,
                  const int32_t* cand, int K, const int32_t* steps, int V, int h, int S, int min_terms,
                  int32_t* best, int32_t* order, int32_t* block, float* ws, void* stream);

/*
 * Pose-graph optimisation of a drive from its odometry and loop-closure edges (csrc/lpd_pgo.hip; arithmetic in csrc/lpd_pgo_math.h):
 * the back end behind lpd_icp_pairs (Grisetti et al., "A tutorial on graph-based SLAM", 2010; Levenberg-Marquardt around block-Jacobi
 * preconditioned conjugate gradients, as Dellaert et al., "Subgraph-preconditioned conjugate gradients", IROS 2010, and g2o's PCG
 * solver do).  This comment is the specification, and lpd_pgo_math.h settles every detail it leaves open.  Everything is float64,
 * every operation rounded once, nothing contracted, + - * / sqrt only, every comparison false on NaN.
 *   G graphs, 1 <= G <= 65535; node_off [G+1], edge_off [G+1] int32 DEVICE arrays rising from 0 to V_total / E_total.  A graph has at
 *            most 65536 nodes and 2^20 edges; an empty graph is legal and left alone; a graph whose offsets do not rise inside the
 *            arrays is left alone as well (status "nothing to do", cost 0).  One workgroup solves one graph, in one launch.
 *   pose     [V_total][12] IN and OUT: the top three rows (R | t) of the node-to-world matrix, the layout of lpd_drive_* and lpd_icp_pairs.
 *   fixed    [V_total] uint8: a non-zero entry is a gauge node that never moves; a graph without one has its node 0 fixed.
 *   edge     [E_total][2] int32 (i, j), LOCAL to the graph; meas [E_total][12] = Z_ij, the measured X_i^-1 X_j; weight [E_total][2] =
 *            (w_rot, w_trans).  An edge is SKIPPED -- neither its measurement nor its weight is read further, it is counted in info --
 *            when an end lies outside its graph, i == j, an entry of meas or weight is not finite, or a weight is negative.
 *   csr_ptr  [V_total+1], csr_idx [2 E_total] int32, the CALLER's: row k lists the ends 2 e + end (e the edge's index in the arrays, end
 *            0 for i, 1 for j) that touch node k (global number).  A node sums its edges in this order.  An entry that names no end
 *            of a used edge of the node's graph at that node is passed over; nothing outside the arrays is read whatever the CSR holds.
 * Residual of an edge: (R_e, t_e) = Z^-1 X_i^-1 X_j; r = (2 sgn(q_w) (q_x, q_y, q_z), t_e), q the unit quaternion of R_e by the branch
 * of the largest of (trace, R00, R11, R22), a tie to the earlier one, sgn(0) = +1.  chi2_e = w_rot |r_rot|^2 + w_trans |r_t|^2; the
 * cost is the sum over the used edges, in the fixed order below, of rho(chi2_e): rho(s) = s for huber = 0, and for huber = d > 0
 * Huber's function of a = sqrt(s), s for a <= d and 2 d a - d^2 beyond, applied as the IRLS factor rho'(s) = d / a on both weights
 * at each linearisation.  A node moves iff it is not fixed and a used edge touches it.
 * Up to `outer` (0 .. 64) Levenberg-Marquardt trials.  A trial: linearise (only after an accepted trial) with the first-order Jacobians
 * of lpd_pgo_jac; solve (H + lambda diag H) x = -g by at most cg_iters (1 .. 1024) iterations of conjugate gradients preconditioned by
 * the damped 6 x 6 diagonal blocks, inverted by lpd_icp_math.h's unpivoted LDL^T, until r'z <= cg_tol^2 (r'z at the start), 0 <=
 * cg_tol < 1; move every node on the right, R_k <- R_k dR(w_k), t_k <- t_k + R_k v_k, dR as in lpd_icp_pairs; evaluate the exact cost.
 * The trial is ACCEPTED iff that cost is below the current one: lambda <- lambda / 10, and the solve has converged when the cost fell
 * by no more than 1e-12 of itself.  Otherwise it is refused: the poses stay bit for bit and lambda <- max(10 lambda, 1e-9).  0 <=
 * lambda0 <= 1e6.  A gradient with r'z = 0 at the start of a trial is convergence as well, and so is a solution with x'x <= 1e-24, which
 * is not applied.
 *   cost     [G][outer+1]: the cost before every trial and at the end; the slots behind the end of the solve repeat the last value.
 *   chi2     [E_total]: the unweighted chi2_e at the final poses; -1 for a skipped edge.
 *   info     [G][8] int32 = (status, trials accepted, trials refused, conjugate-gradient iterations in total, edges used, edges
 *            skipped, nodes moved (0 when no trial was accepted), 0).  status: LPD_PGO_CONVERGED; LPD_PGO_ITERATIONS (the trials ran
 *            out); LPD_PGO_NOTHING (no used edge or no node that moves); LPD_PGO_REFUSED: the first cost, a pivot of a diagonal block,
 *            a solution or a moved pose was not positive / finite -- the solve ends there and the poses are those of the last
 *            accepted trial, bit for bit (the input when none was accepted).
 * Sums: thread t of the 256 takes the edges (nodes) e0 + t, e0 + t + 256, ... in ascending order into one partial; the 256 partials
 * are added by a binary tree (t += t + 128, then 64, ...).  No float atomics: the same bits in every launch.  ws =
 * lpd_pgo_workspace_bytes(V_total, E_total, G) bytes (0: bad sizes), 16-byte aligned, the caller's, one per call in flight, no
 * state between calls.  Every decision is taken on the device; the call only enqueues.
 */
#define LPD_PGO_MAX_NODES 65536
#define LPD_PGO_MAX_EDGES 1048576
#define LPD_PGO_MAX_GRAPHS 65535
#define LPD_PGO_MAX_OUTER 64
#define LPD_PGO_MAX_CG 1024
#define LPD_PGO_CONVERGED 0
#define LPD_PGO_ITERATIONS 1
#define LPD_PGO_NOTHING 2
#define LPD_PGO_REFUSED 3
long long lpd_pgo_workspace_bytes(long long V_total, long long E_total, int G);
int lpd_pgo_solve(double* pose, const uint8_t* fixed, const int32_t* node_off, int V_total, const int32_t* edge, const double* meas,
                  const double* weight, const int32_t* edge_off, int E_total, int G, const int32_t* csr_ptr, const int32_t* csr_idx,
                  int outer, int cg_iters, double cg_tol, double lambda0, double huber, double* cost, double* chi2, int32_t* info,
                  void* ws, void* stream);

/*
 * Pairwise-consistent loop closures: which loops of a graph to hand to lpd_pgo_solve (csrc/lpd_loops.hip; arithmetic in
 * csrc/lpd_loops_math.h; Mangelson et al., "Pairwise consistent measurement set maximization for robust multi-robot map merging", ICRA
 * 2018).  Two loops agree if the cycle through both and the odometry between their ends closes within its uncertainty; a large set of
 * mutually agreeing loops is kept.  This comment is the specification, and lpd_loops_math.h settles every detail it leaves open.
 * Everything is float64, every operation rounded once, nothing contracted, + - * / sqrt only, every comparison false on NaN.
 *   G graphs, 1 <= G <= 65535; node_off [G+1], loop_off [G+1] int32 DEVICE arrays rising from 0 to V_total / P_total, as lpd_pgo_solve
 *            takes them.  A graph holds at most LPD_LOOPS_MAX = 4096 loops.  A row that lies in no graph whose offsets rise inside the
 *            arrays is treated as an invalid loop.
 *   pose     [V_total][12]: the nodes' start, (R | t) row-major.  Read, never written.  The nodes of a graph are consecutive windows, as
 *            the odometry edges link them: between nodes i and k lie |i - k| odometry steps.
 *   edge     [P_total][2] int32 (i, j), LOCAL to the graph; meas [P_total][12] = Z, the measured X_i^-1 X_j; weight [P_total][2] =
 *            (w_rot, w_trans): the loops, as lpd_pgo_solve takes them.
 *   w_or, w_ot  > 0: the weights of ONE odometry step between consecutive nodes; gate >= 0, finite.
 * A loop is VALID iff lpd_pgo_solve would use it (both ends inside the graph and different, meas and weight finite, weights >= 0) and
 * both its weights are > 0.  An invalid loop has an all-zero row and is never chosen.
 * Pair statistic of the valid loops a < b (local numbers) of one graph:
 *   E     = Z_a (X_ja^-1 X_jb) Z_b^-1 (X_ib^-1 X_ia), evaluated as ((Z_a T1) T2), T1 = X_ja^-1 X_jb, T2 = (X_ib Z_b)^-1 X_ia;
 *   r     = (2 sgn(q_w) (q_x, q_y, q_z) of R_E, t_E), the quaternion by lpd_pgo_solve's rule;
 *   n_i   = |i_a - i_b|, n_j = |j_a - j_b|;  c_i^2 = |t(X_ia) - t(X_ib)|^2, c_j^2 = |t(X_ja) - t(X_jb)|^2;
 *   var_r = 1/w_rot,a + 1/w_rot,b + (n_i + n_j) / w_or;
 *   var_t = 1/w_trans,a + 1/w_trans,b + (n_i + n_j) / w_ot + (n_i c_i^2 + n_j c_j^2) / w_or   (the last term is the lever arm: a heading
 *           error at the start of an odometry segment swings the whole chord);
 *   the pair is CONSISTENT iff |r_rot|^2 / var_r + |r_t|^2 / var_t <= gate.
 * Bit (a, b) and bit (b, a) are both the decision for (min, max): the matrix is symmetric by construction; the diagonal is 0.
 *
 * lpd_loop_consistency:
 *   adj      [P_total][ldw] uint64: bit b (the LOCAL loop number; bit b & 63 of word b >> 6) of row a.  Every word is written, zeros
 *            beyond the graph.  1 <= ldw <= 64 is the caller's stride.  A word is one __ballot of 64 lanes (lanes = columns) stored once.
 *   degree   [P_total] int32 = the row's popcount for a valid loop, and -1 for an invalid one: lpd_loop_select needs nothing else to
 *            tell a valid loop that agrees with no other from an invalid one.
 *   A graph with more than 64 ldw loops is left alone: its rows are zero, its degrees -1, and lpd_loop_select reports
 *   LPD_LOOPS_TOO_MANY.  No atomics of any kind.
 *
 * lpd_loop_select takes adj and degree as they are (bits of columns outside the graph, of invalid loops and of the diagonal are masked):
 *   seeds    1 .. LPD_LOOPS_MAX_SEEDS = 64; seed s (from 0) of a graph is the valid loop with the (s+1)-th largest degree, ties to the
 *            lower number, found on the device.  A graph with fewer valid loops runs fewer seeds.
 *   From a seed: C = {seed}, cand = adj[seed].  While cand is not empty: take the u in cand with the largest popcount(adj[u] & cand),
 *   ties to the lowest u; C += u; cand &= adj[u].  Each choice is a block-wide integer maximum of (count << 12) | (4095 - u).  One
 *   workgroup per (graph, seed); no barrier across workgroups of any kind; every loop is bounded by a loop count.  The winner among the
 *   seeds -- the largest C, ties to the lower s -- is chosen in a second small launch enqueued by the same call.  The greedy set is
 *   always maximal (no further loop is consistent with all of it), not always maximum.
 *   accepted [P_total] uint8: 1 for the loops of the winner, 0 for every other loop of a graph; rows of no graph are not written.
 *   info     [G][8] int32 = (status, loops valid, loops chosen, seeds run, the winning seed's loop (-1: none), consistent pairs, 0, 0).
 *            status: LPD_LOOPS_OK; LPD_LOOPS_NOTHING (no valid loop, or offsets that do not rise inside the arrays); LPD_LOOPS_TOO_FEW
 *            (the winner is smaller than min_size >= 1: nothing accepted, 0 chosen); LPD_LOOPS_TOO_MANY (more than 64 ldw loops).
 *   ws       lpd_loop_select_workspace_bytes(G, seeds, ldw) bytes (0: bad sizes), 16-byte aligned, the caller's, one per call in
 *            flight, no state between calls.
 * The same bits in every launch.  Both calls only enqueue; nothing is read back.
 */
#define LPD_LOOPS_MAX 4096
#define LPD_LOOPS_MAX_SEEDS 64
#define LPD_LOOPS_MAX_GRAPHS 65535
#define LPD_LOOPS_OK 0
#define LPD_LOOPS_NOTHING 1
#define LPD_LOOPS_TOO_FEW 2
#define LPD_LOOPS_TOO_MANY 3
int lpd_loop_consistency(const double* pose, const int32_t* node_off, int V_total, const int32_t* edge, const double* meas,
                         const double* weight, const int32_t* loop_off, int P_total, int G, double w_or, double w_ot, double gate,
                         uint64_t* adj, int ldw, int32_t* degree, void* stream);
long long lpd_loop_select_workspace_bytes(int G, int seeds, int ldw);
int lpd_loop_select(const uint64_t* adj, int ldw, const int32_t* degree, const int32_t* loop_off, int P_total, int G, int seeds,
                    int min_size, uint8_t* accepted, int32_t* info, void* ws, void* stream);

/*
 * The drive map (csrc/lpd_map.hip; arithmetic in csrc/lpd_map_math.h): what lpd_pgo_solve's corrected nodes are FOR.  lpd_drive_correct
 * carries the nodes' correction to every scan of the drive, so that the corrected drive goes back into lpd_drive_*; lpd_map_insert
 * averages posed scans into one global voxel grid kept as a hash table -- the product a second lap or session is localised against, and
 * the one quality measure of a loop closure that needs no ground truth: the occupied-cell count falls when the laps coincide.  This
 * comment is the specification, and lpd_map_math.h settles every detail it leaves open.  No read-back.
 *
 * lpd_drive_correct.  Float64; every operation rounded once, nothing contracted; dot products ((a0*b0) + (a1*b1)) + (a2*b2); only
 * + - * / sqrt.
 *   poses      [S][12] float64, the drive's input poses (R | t), the layout of lpd_drive_*
 *   D          [S] int64, the distance of lpd_drive_steps + cumsum, units of 2^-16 m
 *   node_scan  [V] int32, non-decreasing, each in [0, S): the scans that are nodes (a plan's `ref` without the empty windows)
 *   node_pose  [V][12] float64, the optimised nodes
 *   out        [S][12] float64;  info [2] int32, ADDED to: scans made from the nodes, scans passed through
 *  1 Bracket.   a = the last node with node_scan[a] <= i, b = a + 1 the first with node_scan[b] > i; of equal entries a is the last.
 *  2 Node.      i == node_scan[a]: out_i = node_pose[a], a bit copy.
 *  3 Candidate. From a node n at scan s: rel = (R_s^T R_i, R_s^T (t_i - t_s)) of the INPUT poses, the difference first; X' = node_pose[n]
 *               composed with rel (R' = R_n R_rel, t' = R_n t_rel + t_n).  The input odometry stays rigid around the node.
 *  4 One.       Before the first node or behind the last the one candidate is the result.
 *  5 Weight.    alpha = (double)(D_i - D_a) / (double)(D_b - D_a), D_a = D[node_scan[a]]; 0 when the denominator is 0.
 *  6 Blend.     t = t_A + alpha (t_B - t_A).  q_A, q_B = the candidates' quaternions by the largest of (trace, R00, R11, R22)
 *               (lpd_pgo_quat); q_B negated when the four-term dot product is negative; q = q_A + alpha (q_B - q_A), each entry divided by
 *               the square root of the squared norm; R by the usual quadratic form (lpd_map_blend writes it out).
 *  7 Pass.      A scan whose own input pose is not finite, whose bracket involves an input or optimised pose that is not finite, or
 *               whose bracket is not one (node_scan[a] outside [0, i], node_scan[b] outside (i, S)) gets its input pose as a bit copy and
 *               is counted in info[1].  Nothing outside the tables is read, whatever node_scan holds.
 * One thread per scan, a binary search over node_scan, no atomics beyond the two counters: the same bits in every launch.
 * Limits: 1 <= S <= 2^22, 1 <= V <= S.
 *
 * lpd_map_insert.  points / ld / rows / offsets / poses / S as lpd_drive_rows takes them; the scans scan0 .. scan1-1 are inserted.
 *   origin     [3] float64 on the device;  inv_cell fp32 = the caller's 1.0f / cell, 1/16 .. 1024 (a cell of 2^-10 .. 16 m)
 *   keys       [capacity] int64, -1 = an empty slot;  acc [capacity][4] int64 = (Sx, Sy, Sz, m): 32 bytes, a slot's four adds land in
 *              one sector.  capacity a power of two, 16 .. 2^36.  The table is the caller's, and clearing it is the caller's fill.
 *   info       [4] int64, ADDED to: rows inserted, rows dropped, rows lost to a full table, cells created
 *  1 World row. Exactly lpd_drive_rows with frame = 0 and t_ref = origin: M = R_i, u = t_i - origin in float64, the twelve numbers rounded
 *               to fp32 once; w_c = (((M_c0*x) + (M_c1*y)) + (M_c2*z)) + u_c in fp32.  The float64 subtraction first is what keeps a UTM
 *               northing of 5.7e6 usable (there an fp32 ulp is 0.5 m).
 *  2 Cell.      f_c = floorf(w_c * inv_cell); a row with an f_c that is NaN or outside [-2^20, 2^20) is dropped and counted; q_c = (int)
 *               f_c; key = (qx + 2^20) | (qy + 2^20) << 21 | (qz + 2^20) << 42: 63 bits, never -1, ascending key = z-major order.
 *  3 Value.     U_c = (int64) rint((double) w_c * 65536.0), half to even; conversion and product are exact.  |U_c| < 2^41, so the sums of
 *               fewer than 2^22 rows in one cell stay inside an int64 anywhere, of fewer than 2^32 rows within 32 km of the origin.
 *  4 Slot.      The first slot is mix(key) & (capacity - 1), mix = the finaliser of splitmix64 (lpd_map_mix); linear probing with wrap-
 *               around, at most min(128, capacity) probes; compare-and-swap on the key word; on insert or match three 64-bit integer
 *               adds of U and one of 1.  An insert adds 1 to info[3]; running out of probes adds the row to info[2] and the row is lost.
 *  5 Addresses. The only address that comes from data is the masked slot.  Nothing is read unless 0 <= offsets[scan0] <=
 *               offsets[scan1] <= rows; the rows are taken in chunks of 1024 input rows, and a chunk whose part of the offsets table is
 *               not one (lpd_map_chunk_ok: it descends, or does not hold the chunk's rows) is not read and its rows count as dropped.
 * What is and is not deterministic: WHICH slot a key lands in depends on timing.  The mapping key -> (Sx, Sy, Sz, m) does not, as long
 * as info[2] stays 0: integer sums are exact in any order and a key is inserted exactly once.  With info[2] > 0 the table's content is
 * unspecified beyond inserted + dropped + lost == rows of the call; the caller takes a larger table and starts over.  Several calls
 * (batches of scans, a second drive, several streams on several tables) give the same mapping as one call.  By default the rows of a
 * chunk are summed per workgroup in LDS first and each distinct key of the chunk goes to the table once; LPD_DEBUG=map-direct sends every
 * row straight to the table.  Both add the same integers to the same keys.  Integer atomics only; no barrier across workgroups.
 *
 * lpd_map_rehash inserts every occupied slot of a table (keys_in, acc_in, capacity_in) into another one by rule 4, sums and counts as
 * they are: how a table grows.  info as above (rows inserted = the cells' counts m, cells created).
 */
#define LPD_MAP_CHUNK 1024                 /* input rows of one workgroup: chunk c is the rows 1024 c .. 1024 c + 1023 of the table */
#define LPD_MAP_MAX_PROBES 128             /* probes in the caller's table before a row is lost (never more than its capacity) */
#define LPD_MAP_MIN_CAPACITY 16
#define LPD_MAP_MAX_CAPACITY 68719476736   /* 2^36 */
#define LPD_MAP_QLIM 1048576               /* 2^20: a cell index lies in [-2^20, 2^20) */
int lpd_drive_correct(const double* poses, const long long* D, int S, const int32_t* node_scan, const double* node_pose, int V, double* out,
                      int32_t* info, void* stream);
int lpd_map_insert(const float* points, int ld, int rows, const int32_t* offsets, const double* poses, int S, int scan0, int scan1,
                   const double* origin, float inv_cell, long long* keys, long long* acc, long long capacity, long long* info, void* stream);
int lpd_map_rehash(const long long* keys_in, const long long* acc_in, long long capacity_in, long long* keys, long long* acc,
                   long long capacity, long long* info, void* stream);

/*
 * Localisation against the drive map (csrc/lpd_localize.hip; arithmetic in csrc/lpd_loc_math.h): the read side of the hash table that
 * lpd_map_insert fills, and a trimmed point-to-plane ICP of whole posed scans against it -- how a second lap or session is localised
 * against the map of the first.  This comment is the specification, and lpd_loc_math.h settles every detail it leaves open; the world
 * row, cell, key, slot, probe count and cell mean are lpd_map_math.h's, the moments lpd_feat_math.h's, the normal, distance, decisions,
 * quantised row, 29 sums, LDL^T and pose update lpd_icp_math.h's.  No read-back; every call only enqueues.
 *
 * Lookup (both calls; lpd_loc_find).  A key is looked up from lpd_map_slot(key, capacity) on, with wrap-around, for at most
 * lpd_map_probes(capacity) probes: found at the first slot that holds it, absent at the first empty slot or when the probes run out.
 * Keys are never removed, so the answer does not depend on which slot a key landed in.  A neighbour cell with an index outside
 * [-2^20, 2^20) on an axis is absent without a lookup; a found slot with m <= 0 is absent.  The table is READ ONLY here: no insert
 * into it while a call is in flight, and a table that lost rows (its info[2] > 0) is unspecified, as before.
 *
 * lpd_map_surface.  surf [capacity][8] fp32, 16-byte aligned, one 32-byte row a slot = (cx, cy, cz, nx, ny, nz, flatness, cells used);
 * the row of an empty slot is all zeros.  One thread per slot.  For an occupied slot: c = lpd_map_mean of its three sums; the
 * (2 reach + 1)^3 cells around it are visited in ascending dz, dy, dx (ascending key; the cell itself is one of them), reach 1 or 2;
 * for every present one d = c_j - c in fp32 goes into lpd_feat_add, k counts them.  k < min_cells (4 .. (2 reach + 1)^3): normal
 * (0, 0, 0), flatness 0; else (normal, flatness) = lpd_icp_normal(moments, k).  An occupied slot with m <= 0 (no insert makes one) gets
 * (NaN, NaN, NaN, 0, 0, 0, 0, 0): never the nearest of anything.  info [2] int64, ADDED to: slots written with a normal, occupied slots
 * written without one.  The values per key do not depend on slot placement, only their position in surf does.
 *
 * lpd_map_localize.  points / ld / rows / offsets / S / scan0 / scan1 / origin / inv_cell as lpd_map_insert takes them.
 *   keys, surf, capacity   the table and its lpd_map_surface rows (acc is not needed)
 *   pose       [S][12] float64, IN and OUT: only the scans scan0 .. scan1-1 are touched
 *   dmax       HOST array of iters + 1 fp32, each finite, > 0, <= 16;  0 <= iters <= 64;  min_inliers >= 6;  max_flat in (0, 1]
 *   sums       [iters+1][S][32] int64, cleared by the call; the layout of lpd_icp_pairs per (pass, scan)
 *   cell       [rows] int64 or NULL: the LAST pass's corresponding cell key of every row of offsets[scan0] .. offsets[scan1]-1, or -1
 *   info       [S][4] int32, rows scan0 .. scan1-1: (1 for a valid scan else -1, steps applied, steps refused, correspondences of the
 *              last pass)
 *   ws         lpd_map_localize_workspace_bytes(S, iters) bytes, 16-byte aligned
 * A scan is VALID iff its pose is finite, 0 <= offsets[i] <= offsets[i+1] <= rows and it has at most 2^20 rows (2^20 terms of at most
 * 2^40 stay inside an int64).  An invalid scan's pose is left bit for bit, its sums are 0, its rows' cell is -1 and its rows are never
 * read.  The rows are walked as lpd_map_insert walks them (rule 5 there): nothing is read unless 0 <= offsets[scan0] <= offsets[scan1]
 * <= rows, and the rows of a chunk whose part of the offsets table is not one have no correspondence (cell -1).
 * Each pass s runs at the pose that pass s - 1 left:
 *  1 Centre.   Fixed once at entry: g = t_in - origin in float64, g32 = g rounded to fp32.  Residuals are formed around the scan, not
 *              around the map's origin: a lever arm of kilometres would hit the 2^20 clamp of lpd_icp_quant and ruin the conditioning.
 *  2 World row. Exactly the insert's: lpd_map_rel(pose_i, origin) rounded to fp32 once, w_c = lpd_drive_coord(...), so a scan at its
 *              true pose reads exactly the cells it was inserted into; q_c = lpd_map_index(w_c, inv_cell).  A row without a cell has
 *              no correspondence.
 *  3 Correspondence.  Candidates: the 27 cells q + (dx, dy, dz), each offset in -1 .. 1, in ascending dz, dy, dx.  For every present
 *              one d2 = lpd_icp_d2(c, w), c its surf centroid; the running minimum is lpd_icp_nearer (strict: ties go to the lowest
 *              key; a d2 that is not finite never wins).  The winner is the correspondence iff lpd_icp_within(d2, dmax_s), its normal is
 *              not (0, 0, 0) and its flatness <= max_flat.  Only this outcome is specified.  With dmax <= cell no nearer centroid lies
 *              outside the 27 cells; the call does not enforce that.
 *  4 Row.      p = w - g32 and q = c - g32, one fp32 subtraction each; a row with any |p_c| > 512 has no correspondence; then
 *              lpd_icp_row(p, q, n) and lpd_icp_terms, summed in int64: exact in any order.
 *  5 Step.     Passes 0 .. iters-1, float64: lpd_icp_solve's sequence with the rotation about the centre -- T = (t - origin) - g,
 *              (R | T) updated by lpd_icp_update, t = (T' + g) + origin -- refused, the pose left bit for bit, under lpd_icp_solve's
 *              conditions (lpd_loc_step).
 * Integer atomics only: the same bits in every launch, at every capacity and for every slot placement.
 */
#define LPD_LOC_SURF 8                     /* floats of a surf row */
#define LPD_LOC_MAX_ITERS 64
#define LPD_LOC_MAX_SCAN_ROWS 1048576      /* 2^20 rows a scan */
int lpd_map_surface(const long long* keys, const long long* acc, long long capacity, int reach, int min_cells, float* surf, long long* info,
                    void* stream);
long long lpd_map_localize_workspace_bytes(int S, int iters);
int lpd_map_localize(const float* points, int ld, int rows, const int32_t* offsets, int S, int scan0, int scan1, const double* origin,
                     float inv_cell, const long long* keys, const float* surf, long long capacity, const float* dmax, int iters,
                     int min_inliers, float max_flat, double* pose, int32_t* info, long long* sums, long long* cell, void* ws, void* stream);

/*
 * LiDAR odometry (csrc/lpd_odom.hip; arithmetic in csrc/lpd_odom_math.h): scan poses for a drive from its scans alone, in the
 * KISS-ICP style -- a sliding local voxel map and a constant-velocity start.  It is lpd_map_insert and lpd_map_localize run in turn,
 * scan after scan; the calls below are the three things that chain lacked, each made so that the chain never waits for the host.  This
 * comment is the specification, and lpd_odom_math.h settles every detail it leaves open.  Float64 with + - * / sqrt only, every
 * operation rounded once, nothing contracted; integer atomics only; no barrier across workgroups; no read-back; every address that
 * comes from data is masked or checked first; the same bits in every launch.
 *
 * lpd_odom_predict.  pose [S][12] float64 IN and OUT, pred [S][12] float64 OUT (not pose), 0 <= t < S, first_motion [12] float64 on
 * the device or NULL.  One thread.  pred[t] and pose[t] are both set to the start of scan t (lpd_odom_predict_pose):
 *   t == 0   pose[0], a bit copy
 *   t == 1   pose[0], a bit copy; with a first_motion, pose[0] composed with it (lpd_map_compose)
 *   t >= 2   c = lpd_map_candidate(P[t-2], P[t-1], P[t-1]) = P[t-1] (P[t-2]^-1 P[t-1]), its rotation renormalised through the quaternion
 *            exactly as lpd_map_blend(c, c, 0.0) does it.  P[t-1] not finite: that pose, a bit copy -- the scan is then invalid for
 *            lpd_map_localize and counts as lost.  P[t-2] not finite: P[t-1], a bit copy.
 *
 * lpd_odom_accept.  pred, pose as above (pose[t] now holds what lpd_map_localize left); info [S][4] int32 = lpd_map_localize's rows;
 * offsets [S+1] int32, len = offsets[t+1] - offsets[t]; share_q = rint(min_share * 1024) made on the host, 0 .. 1024; max_jump metres,
 * 0 .. 1e6; insert_pose [S][12] float64 OUT; state [S] int32 OUT.  One thread.  Scan t >= 1 is ACCEPTED iff info[t][0] == 1, at least
 * one step was applied (info[t][1] >= 1), len > 0, (int64) info[t][3] * 1024 >= (int64) share_q * len, and the squared translation
 * between pose[t] and pred[t] (the three differences, then lpd_pgo_dot3) is <= max_jump * max_jump.  Scan 0 is accepted iff its pose
 * is finite and len > 0.  Accepted: insert_pose[t] = pose[t], state[t] = 1.  Otherwise: pose[t] = pred[t] bit for bit, insert_pose[t] =
 * twelve NaNs, state[t] = 0 -- lpd_map_insert then drops the scan's rows by its own rule 2, so a lost scan never blurs the map.
 *
 * lpd_map_crop: lpd_map_rehash with a predicate -- the sliding map.  Keys are never removed from a table (the lookup relies on that),
 * so a smaller map is a NEW table.  keys_in / acc_in / capacity_in the old table, keys / acc / capacity the new one (cleared by the
 * caller); centre_pose [12] float64 and origin [3] float64 on the device; inv_cell as lpd_map_insert takes it; 0 <= keep_cells <= 2^21.
 * The centre cell qc is the cell of centre_pose's translation by the insert's own rule: u = (float)(t - origin) (lpd_map_rel), qc_c =
 * lpd_map_index(u_c, inv_cell).  A cell q = unkey(key) goes into the new table, by rule 4 of lpd_map_insert with its sums and count as
 * they are, iff |q_c - qc_c| <= keep_cells on all three axes, in integers.  A centre that is not finite or has no cell keeps every cell.
 * info [5] int64, ADDED to: the first four as lpd_map_rehash (rows = the kept cells' counts, -, rows lost to a full table, cells
 * created), the fifth the cells left behind.  The mapping key -> sums of the kept cells does not depend on slot placement on either side.
 *
 * lpd_map_touch + lpd_map_surface_touched: the surf rows of the cells that an insert changed, and no others.  surf is indexed by slot,
 * and a cell's row depends only on the cells within `reach` of it; so after lpd_map_insert of some scans, lpd_map_touch of the same
 * scans and lpd_map_surface_touched, surf equals a full lpd_map_surface of the same table bit for bit, for any sequence of inserts into
 * one table.  (A new table -- a growth, a crop -- needs the full lpd_map_surface once.)
 *   lpd_map_touch   points .. inv_cell exactly as the lpd_map_insert that went before it; keys / capacity the table AFTER that insert,
 *                   only read; reach 1 or 2; dirty [capacity] bytes.  The rows are walked as lpd_map_insert walks them (rule 5 there) and
 *                   dropped as it drops them (rule 2; a chunk that is not read marks nothing).  For each row's cell q the (2 reach + 1)^3
 *                   cells q + d are looked up (lpd_loc_find) and dirty[slot] = 1 is stored for every one found.
 *   lpd_map_surface_touched   where dirty[slot] is set, surf's row by lpd_loc_surface (lpd_map_surface's own function) and
 *                   dirty[slot] = 0; one thread a MARKED slot (the marked slots of 8192 are gathered per workgroup first).  dirty and surf
 *                   16-byte aligned.  info [2] int64 as lpd_map_surface, ADDED to, for the rows written.
 */
#define LPD_ODOM_SHARE_UNITS 1024          /* share_q counts 1/1024ths of a scan's rows */
#define LPD_ODOM_MAX_KEEP_CELLS 2097152    /* 2^21: beyond it a crop keeps everything anyway */
int lpd_odom_predict(double* pose, double* pred, int S, int t, const double* first_motion, void* stream);
int lpd_odom_accept(const double* pred, double* pose, const int32_t* info, const int32_t* offsets, int S, int t, int share_q, double max_jump,
                    double* insert_pose, int32_t* state, void* stream);
int lpd_map_crop(const long long* keys_in, const long long* acc_in, long long capacity_in, const double* centre_pose, const double* origin,
                 float inv_cell, int keep_cells, long long* keys, long long* acc, long long capacity, long long* info, void* stream);
int lpd_map_touch(const float* points, int ld, int rows, const int32_t* offsets, const double* poses, int S, int scan0, int scan1,
                  const double* origin, float inv_cell, const long long* keys, long long capacity, int reach, unsigned char* dirty, void* stream);
int lpd_map_surface_touched(const long long* keys, const long long* acc, long long capacity, int reach, int min_cells, float* surf,
                            unsigned char* dirty, long long* info, void* stream);

/*
 * Motion compensation of LiDAR sweeps (csrc/lpd_deskew.hip, lpd_odom_motion in csrc/lpd_odom.hip; arithmetic in
 * csrc/lpd_deskew_math.h).  A spinning LiDAR measures the rows of one scan over the whole period of its sweep while the sensor moves;
 * every stage above takes a scan as a rigid snapshot.  lpd_scan_deskew brings every row into the frame the sensor had at ONE time of
 * the sweep, from the time of the row and the motion of the sensor during the sweep -- the first step of KISS-ICP, which takes the
 * motion from the constant-velocity model.  This comment is the specification, and lpd_deskew_math.h settles every detail it leaves
 * open.  Float64 with + - * / sqrt only, every operation rounded once, nothing contracted; integer atomics only; no barrier across
 * workgroups; no read-back; the same bits in every launch.
 *
 * Inputs.  times [rows] fp32, one value a row of the scan table with the row numbering of points: the fraction of the scan's period
 * at which the row was measured, 0 .. 1.  motion [S][12] float64, one rigid motion a scan, row-major 3 x 4: the pose of the sensor at
 * the END of the period in the frame of its START.  ref, a double in 0 .. 1: the time whose frame the scan is brought into (0.5 is
 * KISS-ICP's choice: the middle of the sweep).
 *
 *  1 Row.      a = (double) times[g] - ref; the row (x, y, z) becomes R_a (x, y, z) + a t, where (R_a | a t) =
 *              lpd_map_blend(identity, motion_i, a) of lpd_map_math.h IN EVERY BIT: the normalised blend of the two quaternions and the
 *              linear blend of the translations that lpd_drive_correct uses -- the repository's one definition of a blended pose.  The
 *              three coordinates are float64 dot products in the order of lpd_drive_coord, (((m0 x) + (m1 y)) + (m2 z)) + u, each
 *              rounded to fp32 ONCE.  Under the identity motion the result compares equal to the input.
 *  2 Scan.     What of the blend depends on the scan alone (the motion's quaternion by lpd_pgo_quat, its sign chosen against the
 *              identity's (1, 0, 0, 0), the differences to the identity) is made once a chunk (LpdDeskewScan); a row costs one square
 *              root and four divisions.
 *  3 Passed.   A row whose time does not lie in 0 .. 1 (a NaN does not, -0.0 does) or whose scan's motion holds a value that is not
 *              finite is written as a bit copy of its input and counted in info[1]; info[0] counts the transformed rows.  info [2]
 *              int64, ADDED to, one integer atomic a wave and counter.
 *  4 Walk.     The rows of the scans scan0 .. scan1-1 in chunks of 1024, exactly as lpd_map_insert walks them (rule 5 there): a
 *              chunk that a broken offsets table refuses is neither read nor written nor counted, and nothing outside [0, rows) and
 *              [scan0, scan1] is touched whatever offsets holds.  Rows outside the scans are not written.
 * out [rows][3] fp32, rows contiguous; out may be points itself when ld == 3 (a chunk reads its rows before it writes them).
 *
 * lpd_drive_motions.  poses [S][12] float64 -> motion [S][12] float64 (not poses), one thread a scan: motion[i] =
 * lpd_pgo_between(poses[i], poses[i+1]) packed as a pose; the last scan repeats the motion before it; S == 1 gives the identity.  A pose
 * that is not finite gives a motion that is not finite, whose rows rule 3 passes through and counts.
 *
 * lpd_odom_motion.  One thread, beside lpd_odom_predict: motion[t] = lpd_pgo_between(pose[t-2], pose[t-1]) for t >= 2 -- the motion
 * the constant-velocity start assumes; for t < 2 first_motion [12] (on the device) as it is, the identity when that is NULL.
 */
int lpd_scan_deskew(const float* points, int ld, int rows, const int32_t* offsets, const float* times, const double* motion, int S, int scan0,
                    int scan1, double ref, float* out, long long* info, void* stream);
int lpd_drive_motions(const double* poses, int S, double* motion, void* stream);
int lpd_odom_motion(const double* pose, int S, int t, const double* first_motion, double* motion, void* stream);

/*
 * Moving objects out of the drive map (csrc/lpd_carve.hip; arithmetic in csrc/lpd_carve_math.h).  Every stage above assumes a static
 * world; a car that drives through the scene leaves a trail of cells in the table.  Every row of the scan table is a ray from a known
 * sensor position, and a cell that many later rays pass straight through was not a wall.  lpd_map_pierce counts those rays per occupied
 * cell, lpd_map_carve copies the table without the cells that were pierced often enough, lpd_scan_moving marks the input rows that lie in
 * such a cell.  This comment is the specification, and lpd_carve_math.h settles every detail it leaves open.  The stage never inserts
 * into the table it reads and reads keys, acc and surf only; integer atomics only; no barrier across workgroups; no read-back; every
 * address that comes from data is masked or checked first.  A count belongs to a KEY, not to the slot the key landed in: per key the
 * result is the same bits in every launch, at every capacity, under any batching of scans and on any stream.
 *
 * lpd_map_pierce.  points / ld / rows / offsets / poses / S / scan0 / scan1 / origin / inv_cell / keys / capacity as lpd_map_localize
 * takes them; surf [capacity][8] from lpd_map_surface, 16-byte aligned.
 *   pierce     [capacity] int32, ADDED to: one a ray and pierced cell, at the cell's slot
 *   info       [6] int64, ADDED to: rays traversed, rows dropped, rays cut at max_steps, cells stepped into, cells found, pierces counted
 *   skip_end, skip_start   0 .. 16 cells;  max_steps 1 .. 8192;  max_flat in (0, 1];  clearance, radius in metres, finite, > 0
 *  1 Walk.     The rows are walked as lpd_map_insert walks them (rule 5 there, chunks of 1024); a chunk that is not read counts its rows
 *              as dropped.
 *  2 Ray.      r = lpd_map_rel(pose, origin), the insert's; the endpoint w is the insert's world row, the sensor o = r.u in fp32.  A row
 *              whose endpoint has no cell (lpd_map_index) is dropped; so is every row of a scan whose o has no cell or whose pose is
 *              not finite.
 *  3 Units.    Per axis f = w_c * inv_cell and e = o_c * inv_cell, one fp32 product each -- the product lpd_map_index floors.
 *              A_c = 2 (int64) floor((double) f * 256.0) + 1, B_c likewise from e: units of 1/512 cell, always odd; cell walls are the
 *              multiples of 512, so a point never lies on a wall, and A_c >> 9 == (int) floorf(f).
 *  4 Steps.    D = A - B, s_c = sign(D_c), n = sum |qa_c - qb_c| (qa, qb the cells of A, B).  The next wall of axis c is W_c =
 *              512 (q_c + (s_c > 0)), N_c = |W_c - B_c|.  Each step takes the axis with the smallest N_c / |D_c|, compared by cross-
 *              multiplication N_i |D_j| < N_j |D_i| (both factors below 2^31); ties go to the lowest axis; an axis with D_c == 0 is
 *              never taken.  After a step on axis c: q_c += s_c, N_c += 512.  Exact: no floating point after rule 3.
 *  5 Visits.   The cells visited are those after steps 1 .. min(n - 1, max_steps): neither the sensor's cell nor the endpoint's.  A ray
 *              with n - 1 > max_steps is counted in info[2].  A visited cell nearer than skip_end cells (Chebyshev) to the endpoint's
 *              cell, or nearer than skip_start to the sensor's, is stepped into (info[3]) but not looked up.
 *  6 Pierce.   A visited cell that is looked up and found (lpd_loc_find; info[4]) has the surf row (c, n_c, flat_c, .).  The endpoint's
 *              own cell is looked up once a ray and gives (c_e, n_e, flat_e) or nothing.  A row is RELIABLE iff its normal is not
 *              (0, 0, 0) and its flatness <= max_flat.  Float64 on the fp32 values, every operation rounded once, dot products
 *              ((a0 b0) + (a1 b1)) + (a2 b2).  The cell is pierced iff both hold:
 *                a  the endpoint's row is not reliable, or |n_e . (c - w)| > clearance: the cell does not lie on the surface the ray
 *                   ended on (what stops ground-grazing and wall-grazing rays);
 *                b  the cell's row reliable: g = n_c . (o - c), h = n_c . (w - c), and (g > clearance and h < -clearance) or
 *                   (g < -clearance and h > clearance) -- the ray crosses the cell's plane and ends well behind it;
 *                   else: v = w - o, a = c - o, (a.a)(v.v) - (a.v)^2 < (radius radius)(v.v) -- the ray passes within radius of the
 *                   centroid (no division, no square root).
 *              A comparison with a NaN is false, so a NaN centroid (a slot with m <= 0) never counts.
 * One thread a ray; the walk does not depend on the lookups, so the first probes of the next 8 cells are loaded before any chain is
 * followed; the surf row is loaded only for a found cell.  At most 2^31 - 1 rows may be counted against one table (pierce is int32):
 * the caller's to keep.
 *
 * lpd_map_carve: lpd_map_rehash with a predicate, as lpd_map_crop is.  keys_in / acc_in / capacity_in the old table and pierce
 * [capacity_in] its counts; keys / acc / capacity the new table (cleared by the caller); min_pierce >= 1; ratio_q = rint(ratio * 1024)
 * made on the host, 0 .. 2^20.  A cell of m rows and p pierces is MOVING iff m > 0 and p >= min_pierce and (int64) p * 1024 >=
 * (int64) ratio_q * m (lpd_carve_moving).  Every other occupied cell goes into the new table by rule 4 of lpd_map_insert with its sums and
 * count as they are.  info [5] int64 as lpd_map_crop's: the fifth entry counts the cells left behind.
 *
 * lpd_scan_moving.  The rows as lpd_map_touch takes them, the old table (keys, acc, capacity) and its pierce; min_pierce, ratio_q as
 * above.  flags [rows] uint8: 1 for a row of the scans scan0 .. scan1-1 whose own cell (the insert's rules 1 and 2) is found and MOVING,
 * else 0; a dropped row and a row of a chunk that is not read get 0; rows outside those scans are not written.  info [2] int64, ADDED
 * to: rows flagged, rows not flagged.
 */
#define LPD_CARVE_MAX_SKIP 16              /* skip_end, skip_start: cells */
#define LPD_CARVE_MAX_STEPS 8192           /* cells of one ray that are stepped into */
#define LPD_CARVE_RATIO_UNITS 1024         /* ratio_q counts 1/1024ths of a cell's rows */
#define LPD_CARVE_MAX_RATIO_Q 1048576      /* 2^20 */
int lpd_map_pierce(const float* points, int ld, int rows, const int32_t* offsets, const double* poses, int S, int scan0, int scan1,
                   const double* origin, float inv_cell, const long long* keys, const float* surf, long long capacity, int skip_end,
                   int skip_start, int max_steps, float max_flat, double clearance, double radius, int32_t* pierce, long long* info,
                   void* stream);
int lpd_map_carve(const long long* keys_in, const long long* acc_in, long long capacity_in, const int32_t* pierce, int min_pierce, int ratio_q,
                  long long* keys, long long* acc, long long capacity, long long* info, void* stream);
int lpd_scan_moving(const float* points, int ld, int rows, const int32_t* offsets, const double* poses, int S, int scan0, int scan1,
                    const double* origin, float inv_cell, const long long* keys, const long long* acc, long long capacity, const int32_t* pierce,
                    int min_pierce, int ratio_q, unsigned char* flags, long long* info, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training path (forward in train mode + backward).  What `loss.backward()` does implicitly in the
 * reference (train_pointnetvlad.py:129,158) through BatchNorm batch statistics, LeakyReLU, the max
 * over k, the neighbour gather, softmax and the NetVLAD normalisations; dense products reuse lpd_gemm.
 * fp64 buffers hold the statistics / reduction results ([C] doubles, caller-owned).
 * ------------------------------------------------------------------------------------------------ */

/* Column sums and sums of squares over R rows of X [R][ld] (BatchNorm batch statistics,
 * nn.BatchNorm1d/2d in train mode).  C and ld multiples of 4. */
int lpd_colstats(const float* X, long long ld, long long R, int C, double* sum, double* sumsq, double* stat_ws, void* stream);

/* From the sums: mean, biased variance -> scale = gamma/sqrt(var+eps), shift = beta - mean*scale, mean, invstd;
 * updates running_mean / running_var in place (momentum, unbiased variance) when given. */
int lpd_bn_finalize(const double* sum, const double* sumsq, double count, int C, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float momentum, float eps, float* scale, float* shift,
                    float* mean, float* invstd, void* stream);

/* Y = act(scale * X + shift) elementwise per column (scale/shift NULL = identity affine).  In-place allowed. */
int lpd_affine_act(const float* X, long long ldx, float* Y, long long ldy, long long R, int C, const float* scale,
                   const float* shift, int act, float slope, void* stream);
/* the same with a bf16 copy of the result rows beside the fp32 ones (Y16 [R][ld16] in bf16 elements, ld16 % 4 == 0); Y may be NULL: only
   the bf16 rows are written */
int lpd_affine_act2(const float* X, long long ldx, float* Y, long long ldy, void* Y16, long long ld16, long long R, int C, const float* scale,
                    const float* shift, int act, float slope, void* stream);

/* Backward of Y = act(BN(X)) given dY: dbeta = sum dpre, dgamma = sum dpre*xhat (fp64 [C]) and
 * dX = scale*(dpre - dbeta/R - xhat*dgamma/R); has_bn = 0: plain activation backward (dbeta = bias gradient).
 * X is the raw pre-BatchNorm tensor.  In-place (dX == dY) allowed. */
int lpd_bn_act_bwd(const float* dY, long long lddy, const float* X, long long ldx, float* dX, long long lddx, long long R,
                   int C, const float* scale, const float* shift, const float* mean, const float* invstd, int act,
                   float slope, int has_bn, double* dbeta, double* dgamma, double* stat_ws, void* stream);
/* the same on bf16 tensors (dY, X, dX [R][ld] in bf16 elements, ld % 8 == 0, C a power of two in 8..2048; dX may alias dY): the
 * bf16-storage training mode's conv3 map (util/lpdnet_model.py:262 backward) */
int lpd_bn_act_bwd_bf16(const void* dY, long long lddy, const void* X, long long ldx, void* dX, long long lddx, long long R, int C,
                        const float* scale, const float* shift, const float* mean, const float* invstd, int act, float slope, int has_bn,
                        double* dbeta, double* dgamma, double* stat_ws, void* stream);

/* Materialised edge tensor (training only): U[(i,t)] = P[nbr(i,t)] + Q[i], rows i*k+t, [M*k][C]
 * (the split form of util/lpdnet_model.py:350-357 + the 1x1 conv).  C in {64,128,256}.
 * sum / sumsq ([C] doubles, both or neither): the BatchNorm statistics of U, accumulated while the rows are written
 * (what lpd_colstats would compute in a second pass over U). */
int lpd_edge_build(const float* P, long long ldp, const float* Q, long long ldq, const int32_t* idx, float* U, long long M,
                   int N, int C, int k, double* sum, double* sumsq, double* stat_ws, void* stream);

/* out[i][c] = act(scale[c] * sel_t X[(i,t)][c] + shift[c]) over k consecutive rows (x.max(dim=-1) after
 * BatchNorm + activation, lpdnet_model.py:250,252,258); arg[i][c] = selected t (uint8). */
int lpd_group_max(const float* X, long long ldx, int k, const float* scale, const float* shift, int act, float slope,
                  float* out, long long ldo, uint8_t* arg, long long M, int C, void* stream);
/* The same, also keeping the RAW selected values xsel[i][c] = X[(i,arg[i][c])][c] ([M][ldsel]) for lpd_edge_bn_bwd_sel. */
int lpd_group_max_sel(const float* X, long long ldx, int k, const float* scale, const float* shift, int act, float slope,
                      float* out, long long ldo, uint8_t* arg, float* xsel, long long ldsel, long long M, int C, void* stream);

/* Backward of lpd_group_max w.r.t. the post-activation edge values: dX[(i,arg[i][c])][c] (+)= dOut[i][c];
 * accumulate = 0 writes all k rows (zeros elsewhere). */
int lpd_group_max_bwd(const float* dOut, long long ldo, const uint8_t* arg, int k, float* dX, long long M, int C,
                      int accumulate, void* stream);

/* Fused backward of out[i] = max_t act(BN(X[(i,t)])) on a materialised edge tensor X [M*k][C]: the arg-max gradient
 * comes from (dOut [M][ldo], arg [M][C]); dDense [M*k][C] (optional) is an additional dense gradient on the
 * post-activation edge values (DG1: the DG2 convolution consumes every edge).  Writes dX [M*k][C] (may alias dDense),
 * dQ[i] = sum_t dX[(i,t)] (optional, the centre-term gradient) and the fp64 reductions dbeta/dgamma [C]. */
int lpd_edge_bn_bwd(const float* dOut, long long ldo, const uint8_t* arg, const float* dDense, const float* X, float* dX,
                    float* dQ, long long ldq, int k, long long M, int C, const float* scale, const float* shift,
                    const float* mean, const float* invstd, int act, float slope, float inv_ns, double* dbeta, double* dgamma,
                    double* stat_ws, void* stream);
/* inv_ns (lpd_edge_bn_bwd, lpd_edge_bn_bwd_bf16): 0 = X holds the raw pre-BatchNorm values.  > 0 (dense form, act none / LeakyReLU with
 * negative slope 1 / inv_ns): X holds the POST-activation values Y = act(BN(U)) -- what lpd_edge_mlp_train stores instead of U -- and
 * the pre-activation is recovered as y (y > 0) or y * inv_ns; `mean` then carries the BatchNorm bias beta and `invstd` 1 / gamma
 * (xhat = (pre - beta) / gamma), `scale` stays gamma * invstd.
 * The arg-max-only form (no dense gradient, no dQ) with the raw selected values Xsel [M][ldsel] the forward kept
 * (lpd_group_max_sel): the dbeta / dgamma reduction is an [M][C] pass instead of a gather from the edge tensor. */
int lpd_edge_bn_bwd_sel(const float* dOut, long long ldo, const uint8_t* arg, const float* X, const float* Xsel, long long ldsel,
                        float* dX, int k, long long M, int C, const float* scale, const float* shift, const float* mean,
                        const float* invstd, int act, float slope, double* dbeta, double* dgamma, double* stat_ws, void* stream);

/* dQ[i] = sum_t dU[(i,t)]  (gradient of the centre term). */
int lpd_group_sum(const float* dU, int k, float* dQ, long long ldq, long long M, int C, void* stream);

/* dP[nbr(i,t)] += dU[(i,t)]  (transpose of the neighbour gather; float atomics; dP zeroed by the caller). */
int lpd_scatter_add_rows(const float* dU, const int32_t* idx, float* dP, long long ldp, long long M, int N, int k, int C,
                         void* stream);

/* Transposed kNN graph in CSR form: rowptr [M+1], edges [M*k] (edge id = i*k + t, grouped by the neighbour row they
 * point to); ws: 2*M int32 scratch.  Built once per graph and training step. */
int lpd_graph_transpose(const int32_t* idx, long long M, int N, int k, int32_t* rowptr, int32_t* edges, int32_t* ws,
                        void* stream);
/* dP[j] (+)= sum of dU[e] over the incoming edges e of row j: the same result as lpd_scatter_add_rows without float
 * atomics (each dU row is read once).  dU [M*k][C] contiguous, C in {64,128,256}. */
int lpd_gather_sum_rows(const float* dU, const int32_t* rowptr, const int32_t* edges, float* dP, long long ldp, long long M,
                        int C, int accumulate, void* stream);

/* dW[o][c] = sum_m dY[m][o] * X[m][c] for Kin <= 8 input channels (first layer weight gradient). */
int lpd_dw_smallk(const float* dY, long long lddy, const float* X, long long ldx, long long M, int Co, int Kin, float* dW,
                  void* stream);

/* Per-cloud max over the N points with the arg-max row (first maximum): in [B][N][ld] -> out [B][C], arg [B][C]
 * (train-mode MaxPool2d((num_points,1)) / torch.max(x, 2): util/PointNetVlad.py:162, util/lpdnet_model.py:300). */
int lpd_colmax_arg(const float* in, long long ld, float* out, int32_t* arg, int B, int N, int C, void* stream);

/* Backward of lpd_colmax_arg: dIn[b*N + arg[b][c]][c] = dOut[b][c]; dIn [B*N][ld] zero-filled by the caller. */
int lpd_colmax_bwd(const float* dOut, const int32_t* arg, float* dIn, long long ld, int B, int N, int C, void* stream);

/* Gradient of a per-cloud KD x KD alignment matrix (KD <= 8): dT[b] = sum over the cloud's points of X[m]^T dY[m]
 * (backward of x @ trans, util/lpdnet_model.py:229, util/PointNetVlad.py:209). */
int lpd_cloud_outer(const float* X, long long ldx, const float* dY, long long ldy, float* dT, int B, int N, int KD, void* stream);

/* Softmax backward with the a_sum path folded in: dS = A*(g - sum_c A*g), g = dA + dasum[cloud]. */
int lpd_softmax_bwd(const float* A, const float* dA, const float* dasum, float* dS, long long rows, int ncols,
                    int rows_per_cloud, void* stream);

/* Backward of lpd_vlad_finalize: dVraw [B][F][KC], dasum [B][KC], dcw2 [F][KC] (summed over clouds). */
int lpd_vlad_finalize_bwd(const float* dOut, const float* v, const float* inv_c, const float* inv_g, const float* asum,
                          const float* cw2, float* dVraw, float* dasum, float* dcw2, int B, int F, int KC, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training path, second generation (csrc/lpd_train2.hip).
 * ------------------------------------------------------------------------------------------------ */

/*
 * SPLIT-FORM edge stage in train mode: x3 = max_k act(BN_train(convSN1(cat(f_j, f_i)))) (util/lpdnet_model.py:256-258)
 * without the [M*k][C] edge tensor U[(i,t)] = P[nbr(i,t)] + Q[i].  One gather pass:
 *   S[i] = sum_t P[nbr(i,t)];  usel[i] = sel_t P[nbr(i,t)] + Q[i] (sel = max where gamma[c] >= 0, min where < 0 -- the sign of
 *   the BatchNorm scale), arg[i] = the selected slot;  sum / sumsq [C] doubles = the batch statistics of U in closed form
 *   (sum U = sum_i (S_i + k Q_i), sum U^2 = sum_i (sum_t P_nbr^2 + 2 Q_i S_i + k Q_i^2)) for lpd_bn_finalize with count M*k.
 * x3 = act(scale * usel + shift) is then lpd_affine_act on [M][C].  S, usel [M][C] contiguous; C in {64,128,256}; k <= 255.
 */
int lpd_edge_split_fwd(const float* P, long long ldp, const float* Q, long long ldq, const int32_t* idx, const float* gamma,
                       float* S, float* usel, uint8_t* arg, long long M, int N, int C, int k, double* sum, double* sumsq,
                       double* stat_ws, void* stream);
/*
 * Train-mode DG1 -> DG2 stage in ONE launch (util/lpdnet_model.py:249-252 under batch statistics), replacing
 * lpd_edge_build + lpd_edge_act_max + the [E,128] x [128,128] product + lpd_group_max / lpd_group_sel_stats_bf16:
 *   Y1e[(i,t)][:] = act(s1 (P[nbr(i,t)] + Q[i]) + b1)   (s1 / b1 = BatchNorm1 scale / shift of THIS batch: lpd_edge_split_fwd gives the
 *                   statistics of U = P[nbr] + Q without writing U, and x1 = max_t Y1e with its arg-max through act(s1 usel + b1))
 *   Z = Y1e W2^T (raw), sum / sumsq = its column statistics (fp64, zeroed here), zsel[i][c] = max_t Z (gamma2[c] >= 0) or min_t Z,
 *   arg2[i][c] = the first slot t that attains it.
 * bf16 != 0: Y1e is a bf16 tensor (bf16 storage mode) and the product takes the rounded Y1e (two MFMA products with the split
 * weight); else fp32 and three split-bf16 products.  z_bf16 != 0: Z is stored as bf16 (required with bf16 Y1e, the default with
 * fp32 Y1e too: statistics and selection come from the fp32 accumulators, the stored Z only feeds the backward's xhat2 m2 term).
 * 128 -> 128 channels, M % 64 == 0, N % 64 == 0, k <= 255.
 */
int lpd_edge_mlp_train(const float* P, int ldp, const float* Q, int ldq, const int32_t* idx, const float* s1, const float* b1,
                       const float* W2, const float* gamma2, void* Y1e, void* Z, int bf16, int z_bf16, float* zsel, int ldsel, uint8_t* arg2,
                       double* sum, double* sumsq, int M, int N, int k, int act, float slope, double* stat_ws, void* stream);
/*
 * Backward of the train-mode DG1 -> DG2 stage (the counterpart of lpd_edge_mlp_train), two launches instead of the chain
 * product -> reduce -> apply -> gather over [E,128] tensors:
 *   lpd_edge_mlp_train_bwd: dZ generated from the stored Z while the operand tile is built (A = z a1 + a0 + delta dpre2, cf.
 *     lpd_gemm_bf16s_bnbwd), dY1e = dZ W2 on the MFMA, and in its epilogue G = (dY1e + delta_{t,arg1} dx1) act'(pre1) -- the gradient in
 *     front of BatchNorm1 -- written INSTEAD of dY1e, with dbeta1 = sum G, dgamma1 = sum G xhat1 and gsum[i] = sum_t G[(i,t)];
 *     act' and xhat1 = (pre1 - beta1) rgamma1 come from the stored post-activation Y1e (pre1 = y or y * inv_ns).
 *   lpd_edge_dense_bwd_apply: dP, dQ of U = P[nbr] + Q in closed form from ONE gather pass over the transposed graph (a G row and a Q
 *     row per edge): dP_j = s (sum G - deg m1 - m2 invstd (deg (P_j - mu) + sum Q_i)), dQ_j = s (gsum_j - k m1 - m2 invstd (S_j + k (Q_j - mu))).
 * bf16 != 0: Y1e, dpre2 and G are bf16; z_bf16 != 0: Z is bf16 (as lpd_edge_mlp_train stored it).  M % 32 == 0, 128 channels, k <= 255.
 * Z may be NULL in both calls: lpd_edge_mlp_train then stores no Z, and lpd_edge_mlp_train_bwd forms the dense part of BatchNorm2's
 *     backward as Y1e K (K = W2^T diag(-invstd2 m2 s2) W2, one bf16 product) from `kws` (128 * 128 + 128 floats of caller scratch).
 */
int lpd_edge_mlp_train_bwd(const void* Z, const uint8_t* arg2, const void* dpre2, const float* W2, const float* scale2, const float* mean2,
                           const float* invstd2, const double* dbeta2, const double* dgamma2, const void* Y1e, const uint8_t* arg1,
                           const float* dx1, int lddx1, const float* beta1, const float* rgamma1, int bf16, int z_bf16, void* G, float* gsum,
                           double* dbeta1, double* dgamma1, int M, int k, int act, float slope, float inv_ns, float* kws, double* stat_ws, void* stream);
int lpd_edge_dense_bwd_apply(const void* G, int bf16, const float* gsum, const float* S, const float* P, long long ldp, const float* Q,
                             long long ldq, const int32_t* rowptr, const int32_t* edges, float* dP, long long lddp, float* dQ, long long lddq,
                             long long M, int C, int k, const float* scale, const float* mean, const float* invstd, const double* dbeta,
                             const double* dgamma, void* stream);
/* The same on cloud-resident slices (the organisation of lpd_edge_gather_max16: a block holds an 8-channel slice of a whole cloud in
 * LDS and gathers the k neighbour pieces from there): idx16 from lpd_pack_idx16; k = 20, N <= 4096, C % 8 == 0.  S, usel, arg are
 * bit-identical to lpd_edge_split_fwd, the statistics equal up to the order of the fp64 additions. */
int lpd_edge_split_fwd16_applies(int N, int C, int k);
int lpd_edge_split_fwd16(const float* P, long long ldp, const float* Q, long long ldq, const uint16_t* idx16, const float* gamma, float* S,
                         float* usel, uint8_t* arg, long long M, int N, int C, int k, double* sum, double* sumsq, double* stat_ws, void* stream);

/*
 * Backward of the split-form stage: dOut [M][ldo] = gradient of x3.  half != 0 (bf16 storage, C = 256): the rows the second pass gathers
 * over the transposed graph -- G and Q -- are bf16 copies made by the first pass, kept in the same scratch ([2][M][C] bf16); half & 2:
 * dP / dQ (passed as float*) are bf16 rows as well, lddp / lddq in bf16 elements.
 * G [M][C] (scratch, receives dpre = dOut * act'),
 * dbeta / dgamma [C] doubles (the BatchNorm parameter gradients), dP [M][lddp] and dQ [M][lddq]:
 *   dQ_i = s (dpre_i - k m1 - m2 invstd (S_i + k (Q_i - mu)))
 *   dP_j = s (A_j - deg_j m1 - m2 invstd (deg_j (P_j - mu) + R_j)),  A_j / R_j summed over the incoming edges of j in the
 *   transposed graph (rowptr, edges from lpd_graph_transpose), m1 = dbeta / (M k), m2 = dgamma / (M k).  No float atomics.
 */
int lpd_edge_split_bwd(const float* dOut, long long ldo, const float* usel, const uint8_t* arg, const float* S, const float* P,
                       long long ldp, const float* Q, long long ldq, const int32_t* rowptr, const int32_t* edges, float* G,
                       float* dP, long long lddp, float* dQ, long long lddq, long long M, int C, int k, const float* scale,
                       const float* shift, const float* mean, const float* invstd, int act, float slope, int half, double* dbeta,
                       double* dgamma, double* stat_ws, void* stream);

/*
 * bf16 STORAGE of the per-edge tensors that must exist (BASELINE.json configs[2]: the DG1 -> DG2 chain, where convDG2
 * consumes every post-activation edge, lpdnet_model.py:249-252).  bf16 tensors are uint16_t* ([rows][C] contiguous);
 * statistics, reductions and accumulations stay fp32 / fp64.
 */
/* lpd_edge_build with a bf16 result; the statistics are those of the stored (rounded) values */
int lpd_edge_build_bf16(const float* P, long long ldp, const float* Q, long long ldq, const int32_t* idx, uint16_t* U, long long M,
                        int N, int C, int k, double* sum, double* sumsq, double* stat_ws, void* stream);
/* one pass over U: Y = act(scale U + shift) (bf16, the dense consumer's input) and out[i] = act(scale sel_t U + shift), arg[i] */
/* fp32 storage form of the same pass: Y [M*k][C] = act(scale * U + shift), out [M][ldo] = max over the k rows of a point, arg the slot */
int lpd_edge_act_max(const float* U, int k, const float* scale, const float* shift, int act, float slope, float* Y, float* out,
                     long long ldo, uint8_t* arg, long long M, int C, void* stream);
int lpd_edge_act_max_bf16(const uint16_t* U, int k, const float* scale, const float* shift, int act, float slope, uint16_t* Y,
                          float* out, long long ldo, uint8_t* arg, long long M, int C, void* stream);
/* one pass over the raw conv output Z: batch statistics (sum, sumsq) and the raw selected value sel[i] = sel_t Z[(i,t)] with its
 * slot (max where gamma >= 0, else min); BatchNorm + activation of sel is an [M][C] lpd_affine_act afterwards */
int lpd_group_sel_stats_bf16(const uint16_t* Z, int k, const float* gamma, float* sel, long long lds, uint8_t* arg, long long M, int C,
                             double* sum, double* sumsq, double* stat_ws, void* stream);
/* lpd_edge_bn_bwd on bf16 tensors (dDense optional; dX may alias dDense) */
int lpd_edge_bn_bwd_bf16(const float* dOut, long long ldo, const uint8_t* arg, const uint16_t* dDense, const uint16_t* X, uint16_t* dX,
                         float* dQ, long long ldq, int k, long long M, int C, const float* scale, const float* shift,
                         const float* mean, const float* invstd, int act, float slope, float inv_ns, double* dbeta, double* dgamma,
                         double* stat_ws, void* stream);
/* arg-max-only form with the raw selected values of lpd_group_sel_stats_bf16 (cf. lpd_edge_bn_bwd_sel) */
int lpd_edge_bn_bwd_bf16_sel(const float* dOut, long long ldo, const uint8_t* arg, const uint16_t* X, const float* Xsel, long long ldsel,
                             uint16_t* dX, int k, long long M, int C, const float* scale, const float* shift, const float* mean,
                             const float* invstd, int act, float slope, double* dbeta, double* dgamma, double* stat_ws, void* stream);
/* Backward of x2 = max_k act(BN_train(Z)), Z = Y1e W2^T (lpdnet_model.py:251-252) on bf16 edge tensors WITHOUT the [M*k][128] gradient
 * dZ (csrc/lpd_train3.hip).  (1) dpre16 [M][C] = bf16(dOut * act'(scale Xsel + shift)) and the fp64 sums dbeta = sum dpre,
 * dgamma = sum dpre xhat, from the raw selected values Xsel [M][ldsel] of lpd_group_sel_stats_bf16. */
int lpd_bn_sel_bwd_reduce(const float* dOut, long long ldo, const float* Xsel, long long ldsel, long long M, int C, const float* scale,
                          const float* shift, const float* mean, const float* invstd, int act, float slope, uint16_t* dpre16,
                          double* dbeta, double* dgamma, double* stat_ws, void* stream);
/* (2) dW2 [128][128] = dZ^T Y1e from ONE pass over Y1e [M*k][128] bf16: S = D^T Y1e (D: dpre16 at the arg-max slots), the Gram matrix
 * Y1e^T Y1e and the column sums, then dW2[c] = s_c (S[c] - m1_c s - m2_c invstd_c (W2[c] G - mu_c s)) in fp64.  W2 [128][ldw]: the
 * convolution weight; dbeta / dgamma: the sums of (1); ws: lpd_edge_dw_sel_bf16_ws_bytes(M * k) bytes, 16-byte aligned.
 * Requires (M * k) % 128 == 0, 8 <= k <= 255. */
long long lpd_edge_dw_sel_bf16_ws_bytes(long long E);
int lpd_edge_dw_sel_bf16(const uint16_t* Y, const uint8_t* arg, const uint16_t* dpre16, int k, long long M, const float* W2, long long ldw,
                         const float* scale, const float* mean, const float* invstd, const double* dbeta, const double* dgamma, float* dW2,
                         void* ws, void* stream);
/* (3) dY [M*k][128] (bf16) = dZ W2 with dZ = s (delta dpre - m1 - xhat m2) generated from Z [M*k][128] (bf16), arg [M][128] and dpre16
 * while the operand is loaded.  16 <= k <= 255. */
int lpd_gemm_bf16s_bnbwd(const uint16_t* Z, const uint8_t* arg, const uint16_t* dpre16, int k, long long M, const float* W2, int ldw,
                         const float* scale, const float* mean, const float* invstd, const double* dbeta, const double* dgamma, uint16_t* dY,
                         void* stream);
/* The three steps above for fp32 STORAGE (fp32 Y1e / Z / dY, fp32 dpre; split-bf16 products): (M * k) % 64 == 0, 16 <= k <= 255; the
 * workspace of lpd_edge_dw_sel_f32 is lpd_edge_dw_sel_bf16_ws_bytes(M * k) bytes. */
int lpd_bn_sel_bwd_reduce_f32(const float* dOut, long long ldo, const float* Xsel, long long ldsel, long long M, int C, const float* scale,
                              const float* shift, const float* mean, const float* invstd, int act, float slope, float* dpre, double* dbeta,
                              double* dgamma, double* stat_ws, void* stream);
int lpd_edge_dw_sel_f32(const float* Y, const uint8_t* arg, const float* dpre, int k, long long M, const float* W2, long long ldw,
                        const float* scale, const float* mean, const float* invstd, const double* dbeta, const double* dgamma, float* dW2,
                        void* ws, void* stream);
int lpd_gemm_f32s_bnbwd(const float* Z, const uint8_t* arg, const float* dpre, int k, long long M, const float* W2, int ldw,
                        const float* scale, const float* mean, const float* invstd, const double* dbeta, const double* dgamma, float* dY,
                        void* stream);
/* lpd_gather_sum_rows with a bf16 edge-gradient tensor (fp32 sums) */
int lpd_gather_sum_rows_bf16(const uint16_t* dU, const int32_t* rowptr, const int32_t* edges, float* dP, long long ldp, long long M,
                             int C, int accumulate, void* stream);
/* C [M][N] (bf16) = A [M][K] (bf16) x W, W fp32 [N][ldw] (b_kmajor = 0, torch conv weight) or [K][ldw] (1): the weight is split
 * hi + lo (two products on v_mfma_f32_32x32x16_bf16, fp32 accumulation).  (N, K) in {(128,128), (64,64)}. */
int lpd_gemm_bf16s(const uint16_t* A, const float* W, int ldw, int b_kmajor, uint16_t* C, long long M, int N, int K, void* stream);
/* dW [KA][KB] (fp32) = sum_m A[m][:]^T B[m][:], A [M][KA], B [M][KB] bf16; ws: lpd_gemm_tn_bf16_ws_floats(M, KA, KB) floats */
long long lpd_gemm_tn_bf16_ws_floats(long long M, int KA, int KB);
int lpd_gemm_tn_bf16(const uint16_t* A, const uint16_t* B, float* dW, float* ws, long long M, int KA, int KB, void* stream);

/* dW [KA][KB] (fp32) = sum_m A[m][:]^T B[m][:] for fp32 operands A [M][lda], B [M][ldb] in split-bf16 form (three MFMA products per
 * term, fp32-grade): the weight gradients dW = dY^T X of the training path and, batched over the clouds, the NetVLAD residual
 * pooling act^T x (util/PointNetVlad.py:64-67).  batch problems at strides sA / sB (elements) write dW [batch][KA][KB].
 * KA %% 128 == 0, KB %% 64 == 0; ws: lpd_gemm_tn_ws_floats(M, KA, KB, batch) floats.
 * bf16_rows is a flag word: bit 0 = A holds bf16 rows (lda / sA in bf16 elements; they are the hi image: two products), bit 1 = B holds
 * bf16 rows as well (ldb in bf16 elements; needs bit 0, KA % 256 == 0, KB % 256 == 0, M % 32 == 0, M >= 2048, batch 1): one product per
 * term, exact in the operands.  Products with KA % 256 == 0 over whole 32-row chunks run on row-major LDS images read with
 * ds_read_b64_tr_b16, the others on the register-transposing kernels.
 */
long long lpd_gemm_tn_ws_floats(long long M, int KA, int KB, int batch);
int lpd_gemm_tn(const void* A, long long lda, const float* B, long long ldb, float* dW, float* ws, long long M, int KA, int KB,
                int batch, long long sA, long long sB, int bf16_rows, void* stream);
/* lpd_gemm_tn with the rows of A taken as act(a_scale[a] A[m][a] + a_shift[a]) (multiply, then add: lpd_affine_act's bits; bf16 rows:
 * rounded to bf16 again): a train-mode BatchNorm affine + activation applied where the raw map is staged, so that the activated
 * [B N, 1024] map of util/lpdnet_model.py:262 need not be stored for util/PointNetVlad.py:64-67 (pooling) and the assignment's weight
 * gradient.  KA % 256 == 0, KB % 64 == 0 and KB % 128 != 0, M % 32 == 0, M >= 2048; workspace: lpd_gemm_tn_act_ws_floats. */
long long lpd_gemm_tn_act_ws_floats(long long M, int KA, int KB, int batch, int a_bf16);
int lpd_gemm_tn_act(const void* A, long long lda, const float* B, long long ldb, float* dW, float* ws, long long M, int KA, int KB, int batch,
                    long long sA, long long sB, int a_bf16, const float* a_scale, const float* a_shift, int a_act, float a_slope, void* stream);
/* a_bf16 != 0: A holds bf16 rows (lda, sA in bf16 elements, multiples of 8): two MFMA products per term (bf16-storage training mode). */

/*
 * conv3_lpd of the eval path (util/lpdnet_model.py:262: 512 -> emb_dims per point, + bn3 + activation) on PRE-SPLIT operands:
 *   C[m][n] = act(sum_k A[m][k] W[n][k] + bias[n]),   A = a_hi + a_lo,  three bf16 MFMA products per term (fp32-grade); an
 *   eval-mode BatchNorm rides as W = diag(scale) W_conv, bias = shift
 * a_hi / a_lo: bf16 cloud panels [cloud][K/8][a_panel_ld][8] (hi = bf16(x), lo = bf16(x - hi); written by the producers of
 * [x1 | x2 | x3] or by lpd_split_panels), a_cloud bf16 elements apart; frags: lpd_gemm_prep_b(W [N][K], b_kmajor = 0);
 * C: row-major [M][ldc] (c_cloud = 0) or fp32 cloud panels [cloud][N/8][c_panel_ld][8], c_cloud floats apart.
 * 256 x 256 block tiles, LDS-DMA ring, persistent workgroups (csrc/lpd_gemm_p8.hip).  lpd_gemm_p8_applies: N % 256 == 0,
 * K % 32 == 0, K >= 64, clouds of a multiple of 256 points.  act none / ReLU / LeakyReLU (0 <= slope <= 1).  impl: 0 (= 6) or
 * 5 / 6 staging units in flight.
 */
int lpd_gemm_p8_applies(int M, int N, int K, int panel_n);
int lpd_gemm_p8(const void* a_hi, const void* a_lo, long long a_cloud, int a_panel_ld, const void* frags, float* C, int ldc,
                long long c_cloud, int c_panel_ld, int M, int N, int K, int panel_n, const float* bias,
                int act, float slope, int impl, void* stream);
/* lpd_gemm_p8 + the NetVLAD assignment product (util/PointNetVlad.py:48, x . cluster_weights) of its own output in the same launch:
 * besides C, parts[j][m][0..64) = C[m][256 j .. 256 j + 255] . W2[256 j .. 256 j + 255][0..64) for the N / 256 column blocks j
 * (part_stride floats between the planes); lpd_softmax_affine_parts sums the planes.  w2_frags: lpd_gemm_prep_b(W2 [N][64], ldb,
 * b_kmajor = 1, 64, N). */
int lpd_gemm_p8_fused(const void* a_hi, const void* a_lo, long long a_cloud, int a_panel_ld, const void* frags, float* C, int ldc,
                      long long c_cloud, int c_panel_ld, int M, int N, int K, int panel_n, const float* bias, int act, float slope,
                      const void* w2_frags, float* parts, long long part_stride, void* stream);
/* softmax(scale * (sum of `parts` planes of in, part_stride floats apart) + shift) over 64 columns, with the per-group column sums
 * of lpd_softmax_affine (group_rows % 64 == 0; part: its scratch, rows floats are used); parts in {1, 2, 4, 8} */
int lpd_softmax_affine_parts(const float* in, int parts, long long part_stride, float* out, int rows, const float* scale,
                             const float* shift, int group_rows, float* colsum, int colsum_ld, float* part, void* stream);
/* fp32 cloud panels [clouds][panels][s_panel_ld][8] (s_cloud floats apart) -> the two bf16 planes hi / lo of the same layout
 * ([clouds][panels][d_panel_ld][8], d_cloud elements apart); n rows per panel are converted. */
int lpd_split_panels(const float* src, long long s_cloud, int s_panel_ld, void* hi, void* lo, long long d_cloud, int d_panel_ld,
                     int clouds, int panels, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LPD_HIP_H */
