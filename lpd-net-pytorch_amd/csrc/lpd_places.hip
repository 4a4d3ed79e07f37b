// lpd_places.hip -- place lists from positions on the device: for every query position the database items within a radius, per
// database segment, as sorted CSR rows (what the reference's generating_queries/ makes with KDTree.query_radius on the host:
// generate_training_tuples_baseline.py:52-72 at r = 10 / 50 m, generate_test_sets.py:99-109 at r = 25 m).
// Definition: include/lpd_hip.h; the predicate: lpd_places_math.h.
//
// lpd_radius_count and lpd_radius_fill are ONE templated kernel, a 256-thread workgroup per (16 queries, segment):
//   queries   a wave owns LPD_PLACES_WAVE_QUERIES = 4 query rows of the segment; their positions, self items and liveness are
//             wave-uniform (scalar registers)
//   stage     the workgroup copies the segment's positions into LDS, LPD_PLACES_CHUNK = 1024 at a time (16 KiB, one 16-byte
//             position per thread and trip: ds_write_b128 / ds_read_b128 on consecutive lanes, conflict-free); a chunk starts at
//             seg_off[s] and is masked at the segment's end, so it never straddles two rows
//   test      lane l takes candidate base + l and evaluates the predicate against each of the wave's queries; __ballot gives the
//             members among the 64 candidates
//   count     counter += popcount(ballot), wave-uniform; lane 0 writes counts[g * S + s] at the end
//   fill      a member stores its local index at row base + popcount(ballot & lanes below); row base += popcount(ballot).
//             Candidates are visited in ascending order and lanes are ordered inside a ballot: the rows ascend by construction.
// Both passes run the same instructions on the same predicate; no atomics, no float atomics: the same bits in every launch.
// Six float64 operations per (query, candidate): at four queries per wave the VALU time (96 cycles per 64 candidates and SIMD) is
// six times the LDS read time of the workgroup's four waves (4 cycles per ds_read_b128 each), so four queries per read are enough.
#include <math.h>

#include "lpd_common.h"
#include "lpd_places_math.h"

namespace {

constexpr int PL_T = 256;                              // threads of a workgroup
constexpr int PL_WAVES = PL_T / 64;
constexpr int PL_QW = LPD_PLACES_WAVE_QUERIES;
constexpr int PL_CH = LPD_PLACES_CHUNK;
static_assert(PL_WAVES * PL_QW == LPD_PLACES_BLOCK_QUERIES, "queries of a workgroup");

template <bool FILL>
__global__ __launch_bounds__(PL_T) void radius_kernel(const double2* __restrict__ qpos, int Q, const double2* __restrict__ dpos, int D,
                                                      const int32_t* __restrict__ seg_off, int S, double r2,
                                                      const int32_t* __restrict__ skip_seg, const int32_t* __restrict__ self_item,
                                                      int32_t* __restrict__ counts, const int32_t* __restrict__ row_off,
                                                      int32_t* __restrict__ idx, int nnz)
{
    __shared__ double2 cand[PL_CH];
    const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int a = seg_off[s], e = seg_off[s + 1];      // clipped to the table: nothing outside [0, D) is read
    if (a < 0) a = 0;
    if (e > D) e = D;

    const int g0 = (blockIdx.x * PL_WAVES + wave) * PL_QW;
    double qx[PL_QW], qy[PL_QW];
    int self[PL_QW], n_in[PL_QW];      // n_in: members so far (count), or the place of the row's next entry (fill)
    bool live[PL_QW];
#pragma unroll
    for (int i = 0; i < PL_QW; ++i) {
        const int g = g0 + i;
        live[i] = g < Q && !(skip_seg && skip_seg[g] == s);
        const int gg = g < Q ? g : 0;      // Q >= 1 in every launch
        qx[i] = qpos[gg].x;
        qy[i] = qpos[gg].y;
        self[i] = self_item ? self_item[gg] : -1;
        n_in[i] = FILL && g < Q ? row_off[(long long)g * S + s] : 0;
    }
    const unsigned long long below = (1ull << lane) - 1ull;

    for (int c0 = a; c0 < e; c0 += PL_CH) {      // uniform over the workgroup
        const int n = e - c0 < PL_CH ? e - c0 : PL_CH;
        __syncthreads();      // the previous chunk has been read
        for (int i = tid; i < n; i += PL_T) cand[i] = dpos[c0 + i];
        __syncthreads();
        for (int b = 0; b < n; b += 64) {
            const int k = b + lane;
            const bool have = k < n;
            const double2 p = cand[have ? k : 0];
            const int j = c0 + k;
#pragma unroll
            for (int i = 0; i < PL_QW; ++i) {
                const bool in = have && live[i] && j != self[i] && lpd_place_within(qx[i], qy[i], p.x, p.y, r2);
                const unsigned long long m = __ballot(in);
                if (FILL && in) {
                    const long long at = (long long)n_in[i] + __popcll(m & below);
                    if (at >= 0 && at < nnz) idx[at] = j - a;      // a row_off that is not the scan of the counts cannot write outside idx
                }
                n_in[i] += __popcll(m);
            }
        }
    }
    if (!FILL && lane == 0) {
#pragma unroll
        for (int i = 0; i < PL_QW; ++i)
            if (g0 + i < Q) counts[(long long)(g0 + i) * S + s] = n_in[i];
    }
}

int places_check(const char* name, const double* qpos, int Q, const double* dpos, int D, const int32_t* seg_off, int S, double r)
{
    LPD_CHECK_ARG(Q >= 0 && Q <= LPD_PLACES_MAX_ITEMS && D >= 0 && D <= LPD_PLACES_MAX_ITEMS, "%s: Q=%d D=%d outside 0 .. %d", name, Q, D,
                  LPD_PLACES_MAX_ITEMS);
    LPD_CHECK_ARG(S >= 1 && S <= LPD_PLACES_MAX_SEGMENTS, "%s: S=%d outside 1 .. %d", name, S, LPD_PLACES_MAX_SEGMENTS);
    LPD_CHECK_ARG((long long)Q * S < (1ll << 31), "%s: Q * S = %lld rows, fewer than 2^31 supported", name, (long long)Q * S);
    LPD_CHECK_ARG(isfinite(r) && r >= 0.0, "%s: radius %g (finite, >= 0)", name, r);
    LPD_CHECK_ARG(seg_off && (Q == 0 || qpos) && (D == 0 || dpos), "%s: null pointer", name);
    LPD_CHECK_ARG(((uintptr_t)qpos & 15) == 0 && ((uintptr_t)dpos & 15) == 0, "%s: positions must be 16-byte aligned", name);
    return LPD_OK;
}

}  // namespace

extern "C" int lpd_radius_count(const double* qpos, int Q, const double* dpos, int D, const int32_t* seg_off, int S, double r,
                                const int32_t* skip_seg, const int32_t* self_item, int32_t* counts, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = places_check("lpd_radius_count", qpos, Q, dpos, D, seg_off, S, r);
    if (rc != LPD_OK) return rc;
    LPD_CHECK_ARG(Q == 0 || counts, "lpd_radius_count: null pointer");
    if (Q == 0) return LPD_OK;      // no rows
    const dim3 grid((Q + LPD_PLACES_BLOCK_QUERIES - 1) / LPD_PLACES_BLOCK_QUERIES, S);
    hipLaunchKernelGGL(radius_kernel<false>, grid, dim3(PL_T), 0, stream, reinterpret_cast<const double2*>(qpos), Q,
                       reinterpret_cast<const double2*>(dpos), D, seg_off, S, lpd_place_radius_sq(r), skip_seg, self_item, counts,
                       (const int32_t*)nullptr, (int32_t*)nullptr, 0);
    LPD_CHECK_LAUNCH("lpd_radius_count");
    return LPD_OK;
}

extern "C" int lpd_radius_fill(const double* qpos, int Q, const double* dpos, int D, const int32_t* seg_off, int S, double r,
                               const int32_t* skip_seg, const int32_t* self_item, const int32_t* row_off, int32_t* idx, int nnz,
                               void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = places_check("lpd_radius_fill", qpos, Q, dpos, D, seg_off, S, r);
    if (rc != LPD_OK) return rc;
    LPD_CHECK_ARG(nnz >= 0 && row_off && (nnz == 0 || idx), "lpd_radius_fill: nnz=%d (>= 0), or a null pointer", nnz);
    if (Q == 0 || nnz == 0) return LPD_OK;      // nothing to write
    const dim3 grid((Q + LPD_PLACES_BLOCK_QUERIES - 1) / LPD_PLACES_BLOCK_QUERIES, S);
    hipLaunchKernelGGL(radius_kernel<true>, grid, dim3(PL_T), 0, stream, reinterpret_cast<const double2*>(qpos), Q,
                       reinterpret_cast<const double2*>(dpos), D, seg_off, S, lpd_place_radius_sq(r), skip_seg, self_item, (int32_t*)nullptr,
                       row_off, idx, nnz);
    LPD_CHECK_LAUNCH("lpd_radius_fill");
    return LPD_OK;
}
