// lpd_knn_ws.h -- the layout of the kNN workspace (the `ws` of lpd_knn / lpd_knn_pm: lpd_knn_workspace_floats floats).  Internal.
// knn_ws_layout is the ONLY place that knows the sizes, guards and alignment of the regions: the searches (lpd_knn.hip) and the
// kernels that prepare a workspace for a later search (lpd_front.hip, lpd_morton.hip) take their pointers from it, and the size
// query is its `end`.  DESIGN.md section 4.1 lists the regions with their writers and readers.
#pragma once
#include "lpd_common.h"

namespace {
constexpr int KNN7_MAXN = 65536;      // the best-first search is built for these sizes (BASELINE configs[4]: N = 16384, k = 64)
inline bool knn7_applies(int C, int N, int k) { return C <= 64 && k <= 64 && N <= KNN7_MAXN; }

constexpr int KNN7_XB = 80;          // bf16 per point in the operand image of the low-precision bound pass: 2 halves x 40
constexpr int KNN7_PRE_MAXT = 512;   // that pass runs for clouds of up to 512 tiles (N <= 16384: 16.8 MB of bounds per cloud)
// does the bound pass run for a search with cp floats per operand half?  LPD_DEBUG=knn-pre=0: never (centroid / radius bounds)
inline bool knn7_bound_runs(int cp, int N)
{
    static const bool tight = lpd_debug("knn-pre", 1) != 0;
    return tight && cp == 32 && (N + 31) / 32 <= KNN7_PRE_MAXT;
}

// nt = ceil(N / 32) tiles per cloud; cp = 2 (C <= 4) or 32 (C <= 64).  An absent region is null.
struct KnnWs {
    float* xx;         // [B*N] squared norms
    float* xp;         // [B*N][2][cp] packed operand image; C > 64 (first-generation kernel): absent, the workspace ends behind xx
    // tile statistics and launch order of the best-first search: null where it is not built (knn7_applies); the space stays
    float* cenp;       // [B*nt][2][cp] centroids in packed operand order
    float *cnorm, *rad, *txmax;      // [B*nt] each: |c|^2, radius, max |x|^2; 4 floats of guard behind txmax
    int32_t *pred, *order;           // [B*nt] each: predicted walk length per query tile, launch order; 4 of guard behind order
    // the bound pass: reserved for EVERY cp = 32 search of up to KNN7_PRE_MAXT tiles (1.07 GB at B = 64, N = 16384; nothing with
    // the pass off), although only C = 64 with whole tiles gets xb from the kernels that write the operands (KnnRoute::prep_xb)
    __bf16* xb;        // [B*nt][5][64][8] fragment-major bf16 operand image, at the next 16-byte ADDRESS
    uint16_t* ubq;     // [B*nt][nt][32] bounds (bf16 bits, rounded up)
    float* end;        // base + lpd_knn_workspace_floats(B, C, N, k): fixed, whatever the alignment of xb took
};

// `base` may be null or a dummy (size queries): nothing is dereferenced and the arithmetic is on integers
inline KnnWs knn_ws_layout(int B, int C, int N, int k, float* base)
{
    KnnWs w{};
    const size_t cp = C <= 4 ? 2 : (C <= 64 ? 32 : 0);
    const size_t M = (size_t)B * N, nt = ((size_t)N + 31) / 32, T = (size_t)B * nt;
    uintptr_t p = reinterpret_cast<uintptr_t>(base);
    auto take = [&p](size_t floats) { float* r = reinterpret_cast<float*>(p); p += floats * sizeof(float); return r; };
    w.xx = take(M);
    if (cp) {
        w.xp = take(M * 2 * cp);
        w.cenp = take(T * 2 * cp);
        w.cnorm = take(T);
        w.rad = take(T);
        w.txmax = take(T + 4);
        w.pred = reinterpret_cast<int32_t*>(take(T));
        w.order = reinterpret_cast<int32_t*>(take(T + 4));
        if (knn7_bound_runs((int)cp, N)) {
            const uintptr_t unaligned = p;
            p = (p + 15) & ~(uintptr_t)15;
            w.xb = reinterpret_cast<__bf16*>(take(T * 32 * (KNN7_XB / 2)));
            w.ubq = reinterpret_cast<uint16_t*>(take(T * nt * 16));
            p = unaligned + (T * 32 * (KNN7_XB / 2) + T * nt * 16 + 16) * sizeof(float);      // 16 floats of slack hold the padding
        }
        take(8);      // slack
        if (!knn7_applies(C, N, k)) w = KnnWs{w.xx, w.xp};
    }
    w.end = reinterpret_cast<float*>(p);
    return w;
}

}  // namespace
