// lpd_loops.hip -- pairwise-consistent loop closures before pose-graph optimisation: lpd_loop_consistency and lpd_loop_select.
// include/lpd_hip.h specifies both, csrc/lpd_loops_math.h holds every arithmetic detail, tests/loops_ref.py restates both in numpy.
//
// CONSISTENCY: ONE WAVE PER ROW, ONE BALLOT PER WORD.  Row a of a graph's matrix is the decision of loop a against every loop b of
// the graph.  A wave takes a row; its 64 lanes are 64 columns; each lane evaluates the cycle through (min(a, b), max(a, b)) -- so bit
// (a, b) and bit (b, a) are the same float64 computation and the matrix is symmetric by construction -- and the wave's __ballot is the
// word, stored once by lane 0.  The degree is the sum of the words' popcounts.  No atomics, no LDS, no barrier.
//
// SELECTION: ONE WORKGROUP PER (GRAPH, SEED).  The candidate set and the chosen set are bit rows in LDS.  A step counts, for every
// candidate u, popcount(adj[u] & cand), packs (count, 4095 - u) into one integer, and takes the block-wide maximum, which every thread
// then holds: the control flow is uniform and the choice is a total order, the same in every launch.  Every loop is bounded by a loop
// count.  No barrier crosses workgroups: the winner among the seeds is chosen by a second small launch on the same stream.
#include "lpd_common.h"
#include "lpd_loops_math.h"

#define LC_T 256                          // consistency: four waves, four rows a workgroup
#define LC_WAVES (LC_T / 64)
#define LS_T LPD_LOOPS_THREADS            // selection
#define LS_WAVES (LS_T / 64)

namespace {

struct LcArgs {
    const double* pose;
    const int32_t* node_off;
    const int32_t* edge;
    const double* meas;
    const double* weight;
    const int32_t* loop_off;
    int Vt, Pt, G, ldw;
    double w_or, w_ot, gate;
    uint64_t* adj;
    int32_t* degree;
};

// the last graph g whose first loop is not behind row r (17 halvings cover the 65535 graphs), or -1
__device__ __forceinline__ int lc_graph(const int32_t* off, int G, int r)
{
    if (!(off[0] <= r)) return -1;
    int lo = 0, hi = G;
    for (int step = 0; step < 17 && lo + 1 < hi; ++step) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(LC_T) void loop_consistency_kernel(LcArgs a)
{
    const int lane = threadIdx.x & 63;
    const int r = (int)blockIdx.x * LC_WAVES + ((int)threadIdx.x >> 6);      // the row: one per wave
    if (r >= a.Pt) return;
    uint64_t* row = a.adj + (long long)r * a.ldw;
    const int g = lc_graph(a.loop_off, a.G, r);
    int p0 = 0, P = 0, n0 = 0, V = 0;
    bool ok = false;
    if (g >= 0) {
        p0 = a.loop_off[g];
        const int p1 = a.loop_off[g + 1];
        n0 = a.node_off[g];
        const int n1 = a.node_off[g + 1];
        P = p1 - p0;
        V = n1 - n0;
        ok = p0 >= 0 && p0 <= r && r < p1 && p1 <= a.Pt && P <= 64 * a.ldw && P <= LPD_LOOPS_MAX && n0 >= 0 && n1 >= n0 && n1 <= a.Vt;
    }
    const int la = r - p0;
    const int ia = a.edge[2ll * r], ja = a.edge[2ll * r + 1];
    const double *Za = a.meas + 12ll * r, *wa = a.weight + 2ll * r;
    ok = ok && lpd_loops_valid(ia, ja, V, Za, wa);
    if (!ok) {      // a row of no graph, of a graph that is left alone, or of an invalid loop: all zero, marked
        for (int w = lane; w < a.ldw; w += 64) row[w] = 0ull;
        if (lane == 0) a.degree[r] = -1;
        return;
    }
    const double *Xia = a.pose + 12ll * (n0 + ia), *Xja = a.pose + 12ll * (n0 + ja);
    int deg = 0;
    for (int w = 0; w < a.ldw; ++w) {
        uint64_t word = 0ull;
        if (64 * w < P) {
            const int lb = 64 * w + lane;
            bool bit = false;
            if (lb < P && lb != la) {
                const long long rb = (long long)p0 + lb;
                const int ib = a.edge[2 * rb], jb = a.edge[2 * rb + 1];
                const double *Zb = a.meas + 12 * rb, *wb = a.weight + 2 * rb;
                if (lpd_loops_valid(ib, jb, V, Zb, wb)) {
                    const double *Xib = a.pose + 12ll * (n0 + ib), *Xjb = a.pose + 12ll * (n0 + jb);
                    const bool first = la < lb;      // the statistic is that of (lower loop, higher loop)
                    const double s = lpd_loops_stat(first ? Xia : Xib, first ? Xja : Xjb, first ? Za : Zb, first ? wa : wb, first ? ia : ib,
                                                    first ? ja : jb, first ? Xib : Xia, first ? Xjb : Xja, first ? Zb : Za, first ? wb : wa,
                                                    first ? ib : ia, first ? jb : ja, a.w_or, a.w_ot);
                    bit = lpd_loops_consistent(s, a.gate);
                }
            }
            word = __ballot(bit);
        }
        if (lane == 0) row[w] = word;
        deg += __popcll(word);
    }
    if (lane == 0) a.degree[r] = deg;
}

struct LsArgs {
    const uint64_t* adj;
    const int32_t* degree;
    const int32_t* loop_off;
    int Pt, G, ldw, seeds, min_size;
    uint8_t* accepted;
    int32_t* info;
    uint64_t* rows;      // [G][seeds][ldw]: the set a seed grew
    int32_t* sizes;      // [G][seeds][2] = (its size, the seed's loop or -1)
};

// the maximum of one value per thread; every thread returns it
__device__ __forceinline__ int ls_max(int v, int* red)
{
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(v, o);
        v = other > v ? other : v;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int m = red[0];
    for (int k = 1; k < LS_WAVES; ++k) m = red[k] > m ? red[k] : m;
    __syncthreads();
    return m;
}

__device__ __forceinline__ int ls_sum(int v, int* red)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int m = 0;
    for (int k = 0; k < LS_WAVES; ++k) m += red[k];
    __syncthreads();
    return m;
}

// is this graph's slice of the arrays one the selection works on?  *P = its loops
__device__ __forceinline__ bool ls_graph(const LsArgs& a, int gi, int* p0, int* P, bool* too_many)
{
    *p0 = a.loop_off[gi];
    const int p1 = a.loop_off[gi + 1];
    *P = p1 - *p0;
    const bool sane = *p0 >= 0 && p1 >= *p0 && p1 <= a.Pt;
    *too_many = sane && (*P > 64 * a.ldw || *P > LPD_LOOPS_MAX);
    return sane && !*too_many;
}

__global__ __launch_bounds__(LS_T) void loop_grow_kernel(LsArgs a)
{
    __shared__ int keys[LPD_LOOPS_MAX];
    __shared__ uint64_t cand[64], chosen[64], valid[64];
    __shared__ int red[LS_WAVES];
    const int t = threadIdx.x, s = blockIdx.x, gi = blockIdx.y;
    const long long slot = (long long)gi * a.seeds + s;
    uint64_t* out = a.rows + slot * a.ldw;
    int32_t* size_out = a.sizes + 2 * slot;
    int p0, P;
    bool too_many;
    const bool ok = ls_graph(a, gi, &p0, &P, &too_many);
    int seed = -1;
    if (ok && P > 0) {
        // ---- the keys of the valid loops and their bit row ----
        const int nw = (P + 63) >> 6;
        for (int base = 0; base < 64 * nw; base += LS_T) {      // whole waves: 64 nw <= 4096, a multiple of 64
            const int u = base + t;
            if (u < 64 * nw) {
                int d = u < P ? a.degree[p0 + u] : -1;
                d = d > LPD_LOOPS_MAX - 1 ? LPD_LOOPS_MAX - 1 : d;
                const bool v = d >= 0;
                keys[u] = v ? lpd_loops_key(d, u) : -1;
                const uint64_t m = __ballot(v);
                if ((t & 63) == 0) valid[u >> 6] = m;
            }
        }
        __syncthreads();
        // ---- seed s: the (s + 1)-th largest key ----
        int prev = 0x7fffffff;
        for (int k = 0; k <= s && prev >= 0; ++k) {
            int m = -1;
            for (int u = t; u < P; u += LS_T) {
                const int kk = keys[u];
                if (kk < prev && kk > m) m = kk;
            }
            prev = ls_max(m, red);
        }
        if (prev >= 0) seed = lpd_loops_key_loop(prev);
    }
    if (seed < 0) {      // a graph left alone, without loops, or with fewer than s + 1 valid ones (the same in every thread)
        for (int w = t; w < a.ldw; w += LS_T) out[w] = 0ull;
        if (t == 0) {
            size_out[0] = 0;
            size_out[1] = -1;
        }
        return;
    }
    const int nw = (P + 63) >> 6;
    if (t < 64) {
        const uint64_t self = (t == (seed >> 6)) ? (1ull << (seed & 63)) : 0ull;
        const uint64_t row = t < nw ? a.adj[((long long)p0 + seed) * a.ldw + t] : 0ull;
        cand[t] = t < nw ? (row & valid[t] & lpd_loops_word_mask(t, P) & ~self) : 0ull;
        chosen[t] = self;
    }
    __syncthreads();
    int size = 1;
    for (int it = 0; it < P; ++it) {      // a step takes one loop out of cand: at most P - 1 steps
        int m = -1;
        for (int u = t; u < P; u += LS_T) {      // a thread a candidate: its nw loads are independent and all in flight
            if (!((cand[u >> 6] >> (u & 63)) & 1ull)) continue;
            const uint64_t* row = a.adj + ((long long)p0 + u) * a.ldw;
            int cnt = 0;
            for (int w = 0; w < nw; ++w) cnt += __popcll(row[w] & cand[w]);
            const int k = lpd_loops_key(cnt, u);
            m = k > m ? k : m;
        }
        m = ls_max(m, red);
        if (m < 0) break;
        const int u = lpd_loops_key_loop(m);
        if (t < nw) {
            const uint64_t bit = (t == (u >> 6)) ? (1ull << (u & 63)) : 0ull;
            cand[t] = cand[t] & a.adj[((long long)p0 + u) * a.ldw + t] & ~bit;
            chosen[t] |= bit;
        }
        ++size;
        __syncthreads();
    }
    for (int w = t; w < a.ldw; w += LS_T) out[w] = w < nw ? chosen[w] : 0ull;
    if (t == 0) {
        size_out[0] = size;
        size_out[1] = seed;
    }
}

__global__ __launch_bounds__(LS_T) void loop_pick_kernel(LsArgs a)
{
    __shared__ int red[LS_WAVES];
    const int t = threadIdx.x, gi = blockIdx.x;
    int32_t* info = a.info + 8ll * gi;
    int p0, P;
    bool too_many;
    const bool ok = ls_graph(a, gi, &p0, &P, &too_many);
    if (!ok) {
        if (too_many)
            for (int u = t; u < P; u += LS_T) a.accepted[p0 + u] = 0;
        if (t < 8) info[t] = t == 0 ? (too_many ? LPD_LOOPS_ST_TOO_MANY : LPD_LOOPS_ST_NOTHING) : (t == 4 ? -1 : 0);
        return;
    }
    int nvalid = 0, dsum = 0;
    for (int u = t; u < P; u += LS_T) {
        const int d = a.degree[p0 + u];
        nvalid += d >= 0;
        dsum += d > 0 ? (d > LPD_LOOPS_MAX - 1 ? LPD_LOOPS_MAX - 1 : d) : 0;
    }
    nvalid = ls_sum(nvalid, red);
    dsum = ls_sum(dsum, red);
    const int32_t* sizes = a.sizes + 2ll * gi * a.seeds;
    int best = 0, best_s = -1, run = 0;
    for (int s = 0; s < a.seeds; ++s) {      // the largest set; a tie to the lower seed
        const int sz = sizes[2 * s];
        run += sz > 0;
        if (sz > best) {
            best = sz;
            best_s = s;
        }
    }
    const int status = best_s < 0 ? LPD_LOOPS_ST_NOTHING : (best < a.min_size ? LPD_LOOPS_ST_TOO_FEW : LPD_LOOPS_ST_OK);
    const uint64_t* row = a.rows + ((long long)gi * a.seeds + (best_s < 0 ? 0 : best_s)) * a.ldw;
    for (int u = t; u < P; u += LS_T) a.accepted[p0 + u] = status == LPD_LOOPS_ST_OK ? (uint8_t)((row[u >> 6] >> (u & 63)) & 1ull) : 0;
    if (t == 0) {
        info[0] = status;
        info[1] = nvalid;
        info[2] = status == LPD_LOOPS_ST_OK ? best : 0;
        info[3] = run;
        info[4] = best_s < 0 ? -1 : sizes[2 * best_s + 1];
        info[5] = dsum / 2;
        info[6] = 0;
        info[7] = 0;
    }
}

}      // namespace

extern "C" int lpd_loop_consistency(const double* pose, const int32_t* node_off, int V_total, const int32_t* edge, const double* meas,
                                    const double* weight, const int32_t* loop_off, int P_total, int G, double w_or, double w_ot, double gate,
                                    uint64_t* adj, int ldw, int32_t* degree, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(G >= 1 && G <= LPD_LOOPS_MAX_GRAPHS, "lpd_loop_consistency: G=%d outside 1 .. %d", G, LPD_LOOPS_MAX_GRAPHS);
    LPD_CHECK_ARG(V_total >= 0 && V_total <= (1 << 30) && P_total >= 0 && P_total <= (1 << 24), "lpd_loop_consistency: bad sizes V_total=%d P_total=%d",
                  V_total, P_total);
    LPD_CHECK_ARG(ldw >= 1 && ldw <= LPD_LOOPS_MAX / 64, "lpd_loop_consistency: ldw=%d outside 1 .. %d", ldw, LPD_LOOPS_MAX / 64);
    LPD_CHECK_ARG(node_off && loop_off, "lpd_loop_consistency: null pointer");
    LPD_CHECK_ARG(P_total == 0 || (pose && edge && meas && weight && adj && degree), "lpd_loop_consistency: null loop array");
    LPD_CHECK_ARG(w_or > 0.0 && lpd_icp_finite64(w_or) && w_ot > 0.0 && lpd_icp_finite64(w_ot),
                  "lpd_loop_consistency: odometry weights (%g, %g) (finite, > 0)", w_or, w_ot);
    LPD_CHECK_ARG(gate >= 0.0 && lpd_icp_finite64(gate), "lpd_loop_consistency: gate=%g (finite, >= 0)", gate);
    if (P_total == 0) return LPD_OK;
    LcArgs a;
    a.pose = pose; a.node_off = node_off; a.edge = edge; a.meas = meas; a.weight = weight; a.loop_off = loop_off; a.Vt = V_total;
    a.Pt = P_total; a.G = G; a.ldw = ldw; a.w_or = w_or; a.w_ot = w_ot; a.gate = gate; a.adj = adj; a.degree = degree;
    hipLaunchKernelGGL(loop_consistency_kernel, dim3((unsigned)((P_total + LC_WAVES - 1) / LC_WAVES)), dim3(LC_T), 0, stream, a);
    LPD_CHECK_LAUNCH("lpd_loop_consistency");
    return LPD_OK;
}

extern "C" long long lpd_loop_select_workspace_bytes(int G, int seeds, int ldw)
{
    if (G < 1 || G > LPD_LOOPS_MAX_GRAPHS || seeds < 1 || seeds > LPD_LOOPS_MAX_SEEDS || ldw < 1 || ldw > LPD_LOOPS_MAX / 64) return 0;
    return (long long)G * seeds * (8ll * ldw + 8) + 16;
}

extern "C" int lpd_loop_select(const uint64_t* adj, int ldw, const int32_t* degree, const int32_t* loop_off, int P_total, int G, int seeds,
                               int min_size, uint8_t* accepted, int32_t* info, void* ws, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(G >= 1 && G <= LPD_LOOPS_MAX_GRAPHS, "lpd_loop_select: G=%d outside 1 .. %d", G, LPD_LOOPS_MAX_GRAPHS);
    LPD_CHECK_ARG(P_total >= 0 && P_total <= (1 << 24), "lpd_loop_select: bad size P_total=%d", P_total);
    LPD_CHECK_ARG(ldw >= 1 && ldw <= LPD_LOOPS_MAX / 64, "lpd_loop_select: ldw=%d outside 1 .. %d", ldw, LPD_LOOPS_MAX / 64);
    LPD_CHECK_ARG(seeds >= 1 && seeds <= LPD_LOOPS_MAX_SEEDS, "lpd_loop_select: seeds=%d outside 1 .. %d", seeds, LPD_LOOPS_MAX_SEEDS);
    LPD_CHECK_ARG(min_size >= 1, "lpd_loop_select: min_size=%d (>= 1)", min_size);
    LPD_CHECK_ARG(loop_off && info, "lpd_loop_select: null pointer");
    LPD_CHECK_ARG(P_total == 0 || (adj && degree && accepted), "lpd_loop_select: null loop array");
    LPD_CHECK_ARG(ws && ((uintptr_t)ws & 15) == 0, "lpd_loop_select: the workspace (lpd_loop_select_workspace_bytes, 16-byte aligned) is missing");
    LsArgs a;
    a.adj = adj; a.degree = degree; a.loop_off = loop_off; a.Pt = P_total; a.G = G; a.ldw = ldw; a.seeds = seeds; a.min_size = min_size;
    a.accepted = accepted; a.info = info;
    a.rows = (uint64_t*)ws;
    a.sizes = (int32_t*)(a.rows + (long long)G * seeds * ldw);
    hipLaunchKernelGGL(loop_grow_kernel, dim3((unsigned)seeds, (unsigned)G), dim3(LS_T), 0, stream, a);
    LPD_CHECK_LAUNCH("lpd_loop_select");
    hipLaunchKernelGGL(loop_pick_kernel, dim3((unsigned)G), dim3(LS_T), 0, stream, a);
    LPD_CHECK_LAUNCH("lpd_loop_select");
    return LPD_OK;
}
