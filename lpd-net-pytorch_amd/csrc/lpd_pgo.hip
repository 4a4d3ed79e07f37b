// lpd_pgo.hip -- pose-graph optimisation of a drive from its odometry and loop-closure edges: lpd_pgo_solve.  include/lpd_hip.h
// specifies it, csrc/lpd_pgo_math.h holds every arithmetic detail, tests/pgo_ref.py restates the whole solve in numpy.
//
// ONE WORKGROUP PER GRAPH, THE WHOLE SOLVE IN ONE LAUNCH.  A drive's graph has a few hundred nodes: Levenberg-Marquardt around
// preconditioned conjugate gradients is a chain of small dependent steps, and as launches it would be a thousand of them for microseconds
// of arithmetic each.  Here the 256 threads of a workgroup walk the chain together: an edge phase (thread t takes the edges e0 + t,
// e0 + t + 256, ...) and a node phase (the nodes likewise) alternate, __syncthreads() between them; the vectors, the diagonal blocks and
// the per-edge Jacobians live in the caller's workspace, which only this workgroup touches and which stays in L2 at these sizes.  There
// is no barrier across workgroups of any kind, and every loop is bounded by an argument (outer, cg_iters, the node and edge counts, the
// CSR row lengths clamped to the array).
//
// THE SAME BITS IN EVERY LAUNCH.  A node sums what its edges give it in the order of the caller's CSR; a dot product is each thread's
// partial over its nodes in ascending order, then a fixed binary tree over the 256 partials in LDS.  No float atomics.  Every decision
// (accept, refuse, converge) is a function of such sums, the same in every thread, so the control flow is uniform.
#include <math.h>

#include "lpd_common.h"
#include "lpd_pgo_math.h"

#define PG_T LPD_PGO_THREADS

namespace {

struct PgArgs {
    double* pose;
    const uint8_t* fixed;
    const int32_t* node_off;
    const int32_t* edge;
    const double* meas;
    const double* weight;
    const int32_t* edge_off;
    const int32_t* csr_ptr;
    const int32_t* csr_idx;
    int Vt, Et, G, outer, cg_iters;
    double cg_tol, lambda0, huber;
    double* cost;
    double* chi2;
    int32_t* info;
    // the workspace
    double *pn, *g, *D, *x, *r, *z, *p, *Ap, *jc, *res, *weff, *s;
    int32_t *use, *freen;
};

// sum of one value per thread by a fixed tree; every thread returns the sum
__device__ double pg_sum(double v, double* red)
{
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = PG_T / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = red[t] + red[t + s];
        __syncthreads();
    }
    const double o = red[0];
    __syncthreads();
    return o;
}

__device__ int pg_isum(int v, int* red)
{
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = PG_T / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = red[t] + red[t + s];
        __syncthreads();
    }
    const int o = red[0];
    __syncthreads();
    return o;
}

struct PgGraph { int n0, n1, e0, e1; };

// The edge behind entry q of node k's CSR row, or -1: the entry must name an end (2 e + end) of a used edge of this graph whose
// node is k.  Nothing outside the arrays is read whatever the CSR holds.
__device__ __forceinline__ int pg_entry(const PgArgs& a, const PgGraph& gr, int q, int k, int* end)
{
    const int m = a.csr_idx[q];
    if (m < 2 * gr.e0 || m >= 2 * gr.e1) return -1;      // e1 <= 2^30 is checked by the host: no overflow
    const int e = m >> 1;
    *end = m & 1;
    if (!a.use[e] || a.edge[2 * e + *end] + gr.n0 != k) return -1;
    return e;
}

__device__ __forceinline__ void pg_row(const PgArgs& a, int k, int* q0, int* q1)
{
    int b = a.csr_ptr[k], e = a.csr_ptr[k + 1];
    const int lim = 2 * a.Et;
    b = b < 0 ? 0 : (b > lim ? lim : b);
    e = e < b ? b : (e > lim ? lim : e);
    *q0 = b;
    *q1 = e;
}

// the exact cost at the poses P (the caller's, or the trial poses); chi2_out receives every used edge's unweighted chi-squared
__device__ double pg_cost(const PgArgs& a, const PgGraph& gr, const double* P, double* chi2_out, double* red)
{
    double part = 0.0;
    for (int e = gr.e0 + (int)threadIdx.x; e < gr.e1; e += PG_T) {
        if (!a.use[e]) continue;
        double r[6];
        lpd_pgo_residual(P + 12ll * (gr.n0 + a.edge[2 * e]), P + 12ll * (gr.n0 + a.edge[2 * e + 1]), a.meas + 12ll * e, r);
        const double c = lpd_pgo_chi2(r, a.weight[2 * e], a.weight[2 * e + 1]);
        if (chi2_out) chi2_out[e] = c;
        part = part + lpd_pgo_rho(c, a.huber);
    }
    return pg_sum(part, red);
}

__global__ __launch_bounds__(PG_T) void pgo_solve_kernel(PgArgs a)
{
    __shared__ double red[PG_T];
    __shared__ int ired[PG_T];
    const int t = threadIdx.x, gi = blockIdx.x;
    PgGraph gr = {a.node_off[gi], a.node_off[gi + 1], a.edge_off[gi], a.edge_off[gi + 1]};
    double* cost_out = a.cost + (long long)gi * (a.outer + 1);
    int32_t* info = a.info + 8ll * gi;
    const bool sane = gr.n0 >= 0 && gr.n1 >= gr.n0 && gr.n1 <= a.Vt && gr.n1 - gr.n0 <= LPD_PGO_MAX_NODES && gr.e0 >= 0 && gr.e1 >= gr.e0 &&
                      gr.e1 <= a.Et && gr.e1 - gr.e0 <= LPD_PGO_MAX_EDGES;
    if (!sane) {      // offsets that do not rise inside the arrays: the graph is left alone
        for (int s = t; s <= a.outer; s += PG_T) cost_out[s] = 0.0;
        if (t < 8) info[t] = t == 0 ? LPD_PGO_ST_NOTHING : 0;
        return;
    }
    const int V = gr.n1 - gr.n0;

    // ---- which edges are used, which nodes move ----
    int any_fixed = 0;
    for (int k = gr.n0 + t; k < gr.n1; k += PG_T) any_fixed |= a.fixed[k] != 0;
    any_fixed = __syncthreads_or(any_fixed);
    int used = 0;
    for (int e = gr.e0 + t; e < gr.e1; e += PG_T) {
        const int ok = lpd_pgo_edge_ok(a.edge[2 * e], a.edge[2 * e + 1], V, a.meas + 12ll * e, a.weight + 2ll * e) ? 1 : 0;
        a.use[e] = ok;
        if (!ok) a.chi2[e] = -1.0;
        used += ok;
    }
    used = pg_isum(used, ired);
    int nfree = 0;
    for (int k = gr.n0 + t; k < gr.n1; k += PG_T) {
        int q0, q1, deg = 0, end;
        pg_row(a, k, &q0, &q1);
        for (int q = q0; q < q1; ++q) deg += pg_entry(a, gr, q, k, &end) >= 0;
        const bool fix = a.fixed[k] != 0 || (!any_fixed && k == gr.n0);
        const int fr = !fix && deg > 0;
        a.freen[k] = fr;
        nfree += fr;
    }
    nfree = pg_isum(nfree, ired);

    double cost = pg_cost(a, gr, a.pose, nullptr, red);
    if (t == 0) cost_out[0] = cost;
    int status = LPD_PGO_ST_ITERATIONS, accepted = 0, refused = 0, cg_total = 0;
    bool done = false, relin = true;
    double lambda = a.lambda0;
    if (used == 0 || nfree == 0) {
        status = LPD_PGO_ST_NOTHING;
        done = true;
    } else if (!lpd_icp_finite64(cost)) {
        status = LPD_PGO_ST_REFUSED;
        done = true;
    }

    for (int it = 0; it < a.outer; ++it) {
        if (!done) {
            if (relin) {
                // ---- linearise: the edges' residuals and Jacobians, then every node's gradient and diagonal block ----
                for (int e = gr.e0 + t; e < gr.e1; e += PG_T) {
                    if (!a.use[e]) continue;
                    double r[6];
                    lpd_pgo_edge(a.pose + 12ll * (gr.n0 + a.edge[2 * e]), a.pose + 12ll * (gr.n0 + a.edge[2 * e + 1]), a.meas + 12ll * e,
                                 a.jc + 36ll * e, r);
                    for (int c = 0; c < 6; ++c) a.res[6ll * e + c] = r[c];
                    const double f = lpd_pgo_irls(lpd_pgo_chi2(r, a.weight[2 * e], a.weight[2 * e + 1]), a.huber);
                    a.weff[2ll * e] = a.weight[2 * e] * f;
                    a.weff[2ll * e + 1] = a.weight[2 * e + 1] * f;
                }
                __syncthreads();
                for (int k = gr.n0 + t; k < gr.n1; k += PG_T) {
                    double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, D[21];
                    for (int c = 0; c < 21; ++c) D[c] = 0.0;
                    if (a.freen[k]) {
                        int q0, q1, end;
                        pg_row(a, k, &q0, &q1);
                        for (int q = q0; q < q1; ++q) {
                            const int e = pg_entry(a, gr, q, k, &end);
                            if (e < 0) continue;
                            double J[36], s[6], o[6], blk[21];
                            lpd_pgo_jac(a.jc + 36ll * e, end, J);
                            lpd_pgo_wr(a.res + 6ll * e, a.weff + 2ll * e, s);
                            lpd_pgo_jt(J, s, o);
                            lpd_pgo_jtwj(J, a.weff + 2ll * e, blk);
                            for (int c = 0; c < 6; ++c) g[c] = g[c] + o[c];
                            for (int c = 0; c < 21; ++c) D[c] = D[c] + blk[c];
                        }
                    }
                    for (int c = 0; c < 6; ++c) a.g[6ll * k + c] = g[c];
                    for (int c = 0; c < 21; ++c) a.D[21ll * k + c] = D[c];
                }
                relin = false;
            }
            // ---- conjugate gradients on (H + lambda diag H) x = -g, preconditioned by the damped diagonal blocks ----
            double part = 0.0;
            int bad = 0;
            for (int k = gr.n0 + t; k < gr.n1; k += PG_T) {
                double r[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, z[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                if (a.freen[k]) {
                    for (int c = 0; c < 6; ++c) r[c] = -a.g[6ll * k + c];
                    if (!lpd_pgo_precond(a.D + 21ll * k, lambda, r, z)) bad = 1;
                    part = part + lpd_pgo_dot6(r, z);
                }
                for (int c = 0; c < 6; ++c) {
                    a.r[6ll * k + c] = r[c];
                    a.z[6ll * k + c] = z[c];
                    a.p[6ll * k + c] = z[c];
                    a.x[6ll * k + c] = 0.0;
                }
            }
            bad = __syncthreads_or(bad);
            double rz = pg_sum(part, red);
            if (bad || !lpd_icp_finite64(rz)) {
                status = LPD_PGO_ST_REFUSED;
                done = true;
            } else if (!(rz > 0.0)) {      // no gradient left
                status = LPD_PGO_ST_CONVERGED;
                done = true;
            }
            if (!done) {
                const double rz0 = rz;
                for (int n = 0; n < a.cg_iters; ++n) {
                    for (int e = gr.e0 + t; e < gr.e1; e += PG_T) {
                        if (!a.use[e]) continue;
                        double s[6];
                        lpd_pgo_ju(a.jc + 36ll * e, a.weff + 2ll * e, a.p + 6ll * (gr.n0 + a.edge[2 * e]), a.p + 6ll * (gr.n0 + a.edge[2 * e + 1]), s);
                        for (int c = 0; c < 6; ++c) a.s[6ll * e + c] = s[c];
                    }
                    __syncthreads();
                    part = 0.0;
                    for (int k = gr.n0 + t; k < gr.n1; k += PG_T) {
                        if (!a.freen[k]) continue;      // Ap stays unread: p, r and z of such a node are 0 throughout
                        double Ap[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, p[6];
                        int q0, q1, end;
                        pg_row(a, k, &q0, &q1);
                        for (int q = q0; q < q1; ++q) {
                            const int e = pg_entry(a, gr, q, k, &end);
                            if (e < 0) continue;
                            double J[36], o[6];
                            lpd_pgo_jac(a.jc + 36ll * e, end, J);
                            lpd_pgo_jt(J, a.s + 6ll * e, o);
                            for (int c = 0; c < 6; ++c) Ap[c] = Ap[c] + o[c];
                        }
                        for (int c = 0; c < 6; ++c) {
                            p[c] = a.p[6ll * k + c];
                            Ap[c] = Ap[c] + ((lambda * lpd_pgo_diag(a.D + 21ll * k, c)) * p[c]);
                            a.Ap[6ll * k + c] = Ap[c];
                        }
                        part = part + lpd_pgo_dot6(p, Ap);
                    }
                    const double pAp = pg_sum(part, red);
                    if (!(pAp > 0.0 && lpd_icp_finite64(pAp))) break;
                    const double al = rz / pAp;
                    part = 0.0;
                    bad = 0;
                    for (int k = gr.n0 + t; k < gr.n1; k += PG_T) {
                        if (!a.freen[k]) continue;
                        double r[6], z[6];
                        for (int c = 0; c < 6; ++c) {
                            a.x[6ll * k + c] = a.x[6ll * k + c] + (al * a.p[6ll * k + c]);
                            r[c] = a.r[6ll * k + c] - (al * a.Ap[6ll * k + c]);
                            a.r[6ll * k + c] = r[c];
                        }
                        if (!lpd_pgo_precond(a.D + 21ll * k, lambda, r, z)) {
                            bad = 1;
                            continue;
                        }
                        for (int c = 0; c < 6; ++c) a.z[6ll * k + c] = z[c];
                        part = part + lpd_pgo_dot6(r, z);
                    }
                    bad = __syncthreads_or(bad);
                    const double rz2 = pg_sum(part, red);
                    ++cg_total;
                    if (bad) {
                        status = LPD_PGO_ST_REFUSED;
                        done = true;
                        break;
                    }
                    if (!lpd_pgo_cg_continue(rz2, rz0, a.cg_tol)) break;
                    const double be = rz2 / rz;
                    for (int k = gr.n0 + t; k < gr.n1; k += PG_T) {
                        if (!a.freen[k]) continue;
                        for (int c = 0; c < 6; ++c) a.p[6ll * k + c] = a.z[6ll * k + c] + (be * a.p[6ll * k + c]);
                    }
                    rz = rz2;
                    __syncthreads();
                }
            }
            // ---- the trial step and its exact cost ----
            if (!done) {      // a step below XTOL in norm is not taken: converged (a graph whose cost goes to 0 never meets FTOL)
                part = 0.0;
                for (int k = gr.n0 + t; k < gr.n1; k += PG_T)
                    if (a.freen[k]) part = part + lpd_pgo_dot6(a.x + 6ll * k, a.x + 6ll * k);
                if (lpd_pgo_small_step(pg_sum(part, red))) {
                    status = LPD_PGO_ST_CONVERGED;
                    done = true;
                }
            }
            if (!done) {
                bad = 0;
                for (int k = gr.n0 + t; k < gr.n1; k += PG_T) {
                    double out[12];
                    if (a.freen[k]) {
                        if (!lpd_pgo_retract(a.pose + 12ll * k, a.x + 6ll * k, out)) bad = 1;
                    } else {
                        for (int c = 0; c < 12; ++c) out[c] = a.pose[12ll * k + c];
                    }
                    for (int c = 0; c < 12; ++c) a.pn[12ll * k + c] = out[c];
                }
                bad = __syncthreads_or(bad);
                if (bad) {
                    status = LPD_PGO_ST_REFUSED;
                    done = true;
                }
            }
            if (!done) {
                const double trial = pg_cost(a, gr, a.pn, nullptr, red);
                if (lpd_pgo_accept(cost, trial)) {
                    for (int k = gr.n0 + t; k < gr.n1; k += PG_T) {
                        if (!a.freen[k]) continue;
                        for (int c = 0; c < 12; ++c) a.pose[12ll * k + c] = a.pn[12ll * k + c];
                    }
                    __syncthreads();
                    if (lpd_pgo_converged(cost, trial)) {
                        status = LPD_PGO_ST_CONVERGED;
                        done = true;
                    }
                    cost = trial;
                    ++accepted;
                    lambda = lpd_pgo_lambda_down(lambda);
                    relin = true;
                } else {
                    ++refused;
                    lambda = lpd_pgo_lambda_up(lambda);
                }
            }
        }
        if (t == 0) cost_out[it + 1] = cost;
    }
    pg_cost(a, gr, a.pose, a.chi2, red);
    if (t == 0) {
        info[0] = status;
        info[1] = accepted;
        info[2] = refused;
        info[3] = cg_total;
        info[4] = used;
        info[5] = (gr.e1 - gr.e0) - used;
        info[6] = accepted > 0 ? nfree : 0;
        info[7] = 0;
    }
}

}      // namespace

extern "C" long long lpd_pgo_workspace_bytes(long long V_total, long long E_total, int G)
{
    if (V_total < 0 || E_total < 0 || G < 1 || G > LPD_PGO_MAX_GRAPHS || V_total > (1ll << 30) || E_total > (1ll << 29)) return 0;
    const long long b = 8 * (LPD_PGO_NODE_WS * V_total + LPD_PGO_EDGE_WS * E_total) + 4 * (V_total + E_total);
    return (b + 15) / 16 * 16 + 16;
}

extern "C" int lpd_pgo_solve(double* pose, const uint8_t* fixed, const int32_t* node_off, int V_total, const int32_t* edge, const double* meas,
                             const double* weight, const int32_t* edge_off, int E_total, int G, const int32_t* csr_ptr, const int32_t* csr_idx,
                             int outer, int cg_iters, double cg_tol, double lambda0, double huber, double* cost, double* chi2, int32_t* info,
                             void* ws, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(G >= 1 && G <= LPD_PGO_MAX_GRAPHS, "lpd_pgo_solve: G=%d outside 1 .. %d", G, LPD_PGO_MAX_GRAPHS);
    LPD_CHECK_ARG(V_total >= 0 && V_total <= (1 << 30) && E_total >= 0 && E_total <= (1 << 29), "lpd_pgo_solve: bad sizes V_total=%d E_total=%d", V_total,
                  E_total);
    LPD_CHECK_ARG(node_off && edge_off && cost && info, "lpd_pgo_solve: null pointer");
    LPD_CHECK_ARG(V_total == 0 || (pose && fixed && csr_ptr), "lpd_pgo_solve: null node array");
    LPD_CHECK_ARG(E_total == 0 || (edge && meas && weight && csr_idx && chi2), "lpd_pgo_solve: null edge array");
    LPD_CHECK_ARG(outer >= 0 && outer <= LPD_PGO_MAX_OUTER, "lpd_pgo_solve: outer=%d outside 0 .. %d", outer, LPD_PGO_MAX_OUTER);
    LPD_CHECK_ARG(cg_iters >= 1 && cg_iters <= LPD_PGO_MAX_CG, "lpd_pgo_solve: cg_iters=%d outside 1 .. %d", cg_iters, LPD_PGO_MAX_CG);
    LPD_CHECK_ARG(cg_tol >= 0.0 && cg_tol < 1.0, "lpd_pgo_solve: cg_tol=%g outside [0, 1)", cg_tol);
    LPD_CHECK_ARG(lambda0 >= 0.0 && lambda0 <= 1e6, "lpd_pgo_solve: lambda0=%g outside [0, 1e6]", lambda0);
    LPD_CHECK_ARG(huber >= 0.0 && lpd_icp_finite64(huber), "lpd_pgo_solve: huber=%g (finite, >= 0)", huber);
    LPD_CHECK_ARG(ws && ((uintptr_t)ws & 15) == 0, "lpd_pgo_solve: the workspace (lpd_pgo_workspace_bytes, 16-byte aligned) is missing");
    PgArgs a;
    a.pose = pose; a.fixed = fixed; a.node_off = node_off; a.edge = edge; a.meas = meas; a.weight = weight; a.edge_off = edge_off;
    a.csr_ptr = csr_ptr; a.csr_idx = csr_idx; a.Vt = V_total; a.Et = E_total; a.G = G; a.outer = outer; a.cg_iters = cg_iters;
    a.cg_tol = cg_tol; a.lambda0 = lambda0; a.huber = huber; a.cost = cost; a.chi2 = chi2; a.info = info;
    const long long V = V_total, E = E_total;
    double* w = (double*)ws;
    a.pn = w; w += 12 * V;
    a.g = w; w += 6 * V;
    a.D = w; w += 21 * V;
    a.x = w; w += 6 * V;
    a.r = w; w += 6 * V;
    a.z = w; w += 6 * V;
    a.p = w; w += 6 * V;
    a.Ap = w; w += 6 * V;
    a.jc = w; w += 36 * E;
    a.res = w; w += 6 * E;
    a.weff = w; w += 2 * E;
    a.s = w; w += 6 * E;
    a.use = (int32_t*)w;
    a.freen = a.use + E;
    hipLaunchKernelGGL(pgo_solve_kernel, dim3((unsigned)G), dim3(PG_T), 0, stream, a);
    LPD_CHECK_LAUNCH("lpd_pgo_solve");
    return LPD_OK;
}
