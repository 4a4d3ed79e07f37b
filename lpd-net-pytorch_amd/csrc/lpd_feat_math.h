// lpd_feat_math.h -- the per-point arithmetic of lpd_local_features (csrc/lpd_feat.hip): centred neighbourhood moments ->
// covariance -> eigenvalues (cyclic Jacobi, fixed count) -> the ten local point-distribution features of include/lpd_hip.h.
//
// Plain fp32 C++, no HIP types: the kernel includes it for the device, and a host compiler can include it unchanged to run the
// same arithmetic against an fp64 reference without a GPU (every function is a pure function of its arguments).
#pragma once
#include <float.h>
#include <math.h>

#if defined(__HIPCC__)
#define LPD_FEAT_FN __host__ __device__ __forceinline__
#else
#define LPD_FEAT_FN static inline
#endif

#define LPD_FEAT_COLUMNS 10
#define LPD_FEAT_SWEEPS 6      // six sweeps of three rotations reproduce fp64 eigh to ~1e-6 on the eigenvalue ratios

// Sums over the first k list entries of d_j = x_{n_j} - x_i.  Centred on the query point: the entries are of the size of the
// neighbourhood, so the products do not carry the cloud's offset from the origin (raw-coordinate moments of a cloud at (100, -50, 20)
// lose every digit of the covariance in fp32).
struct LpdFeatMoments {
    float sx, sy, sz, sxx, sxy, sxz, syy, syz, szz;
    float zmin, zmax;      // of d_j.z
    float r2;              // |d_{k-1}|^2: the list is sorted nearest-first, so this is the neighbourhood's squared radius
};

LPD_FEAT_FN void lpd_feat_init(LpdFeatMoments& m)
{
    m.sx = m.sy = m.sz = m.sxx = m.sxy = m.sxz = m.syy = m.syz = m.szz = 0.0f;
    m.zmin = INFINITY;
    m.zmax = -INFINITY;
    m.r2 = 0.0f;
}

LPD_FEAT_FN void lpd_feat_add(LpdFeatMoments& m, float dx, float dy, float dz)
{
    m.sx += dx;
    m.sy += dy;
    m.sz += dz;
    m.sxx += dx * dx;
    m.sxy += dx * dy;
    m.sxz += dx * dz;
    m.syy += dy * dy;
    m.syz += dy * dz;
    m.szz += dz * dz;
    m.zmin = fminf(m.zmin, dz);
    m.zmax = fmaxf(m.zmax, dz);
    m.r2 = dx * dx + dy * dy + dz * dz;
}

struct LpdFeatCov { float xx, yy, zz, xy, xz, yz; };

// S = (1/k) sum d d^T - mu mu^T
LPD_FEAT_FN LpdFeatCov lpd_feat_cov(const LpdFeatMoments& m, int k)
{
    const float kf = (float)k;
    const float mx = m.sx / kf, my = m.sy / kf, mz = m.sz / kf;
    LpdFeatCov S;
    S.xx = m.sxx / kf - mx * mx;
    S.yy = m.syy / kf - my * my;
    S.zz = m.szz / kf - mz * mz;
    S.xy = m.sxy / kf - mx * my;
    S.xz = m.sxz / kf - mx * mz;
    S.yz = m.syz / kf - my * mz;
    return S;
}

// One Jacobi rotation in the (p, q) plane of a symmetric 3x3 matrix; r is the third index.  vp / vq: the entries of ONE row of the
// accumulated eigenvector matrix (the z row: all that |n_z| needs).  A zero off-diagonal entry leaves everything bit for bit as it is
// (t = 0, c = 1, s = 0), so exact structure -- a cloud in the plane z = 0 -- survives the sweeps.
LPD_FEAT_FN void lpd_feat_rotate(float& app, float& aqq, float& apq, float& arp, float& arq, float& vp, float& vq)
{
    const float theta = (aqq - app) / (2.0f * apq);
    const float tt = copysignf(1.0f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.0f));      // theta = +-inf: 0
    const float t = apq == 0.0f ? 0.0f : tt;
    const float c = 1.0f / sqrtf(t * t + 1.0f), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0f;
    const float rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp;
    arq = rq;
    const float wp = c * vp - s * vq, wq = s * vp + c * vq;
    vp = wp;
    vq = wq;
}

struct LpdFeatEig {
    float l1, l2, l3;      // descending, clamped at 0
    float nz;              // z component of the unit eigenvector of l3
};

// Fixed-count cyclic Jacobi: backward-stable in fp32 (every step is an orthogonal similarity), no branches on the data.
LPD_FEAT_FN LpdFeatEig lpd_feat_eig(const LpdFeatCov& S)
{
    float a0 = S.xx, a1 = S.yy, a2 = S.zz, a01 = S.xy, a02 = S.xz, a12 = S.yz;
    float v0 = 0.0f, v1 = 0.0f, v2 = 1.0f;      // row z of V = I
#if defined(__clang__)
#pragma unroll 1
#endif
    for (int sweep = 0; sweep < LPD_FEAT_SWEEPS; ++sweep) {
        lpd_feat_rotate(a0, a1, a01, a02, a12, v0, v1);      // (0, 1), r = 2
        lpd_feat_rotate(a0, a2, a02, a01, a12, v0, v2);      // (0, 2), r = 1
        lpd_feat_rotate(a1, a2, a12, a01, a02, v1, v2);      // (1, 2), r = 0
    }
    LpdFeatEig e;
    e.l1 = fmaxf(fmaxf(a0, fmaxf(a1, a2)), 0.0f);
    e.l3 = fmaxf(fminf(a0, fminf(a1, a2)), 0.0f);
    e.l2 = fmaxf(fmaxf(fminf(a0, a1), fminf(fmaxf(a0, a1), a2)), 0.0f);      // the median
    e.nz = (a0 <= a1 && a0 <= a2) ? v0 : (a1 <= a2 ? v1 : v2);
    return e;
}

LPD_FEAT_FN float lpd_feat_xlogx(float e) { return e > 0.0f ? e * logf(e) : 0.0f; }      // 0 ln 0 = 0

// eigenentropy A = -sum e_i ln e_i of the normalised eigenvalues (0 for a neighbourhood without extent)
LPD_FEAT_FN float lpd_feat_entropy(const LpdFeatEig& e)
{
    const float s = e.l1 + e.l2 + e.l3;
    if (!(s > 0.0f)) return 0.0f;
    return -(lpd_feat_xlogx(e.l1 / s) + lpd_feat_xlogx(e.l2 / s) + lpd_feat_xlogx(e.l3 / s));
}

// The ten columns (include/lpd_hip.h) of a neighbourhood of k points.
LPD_FEAT_FN void lpd_feat_columns(const LpdFeatMoments& m, int k, float f[LPD_FEAT_COLUMNS])
{
    const LpdFeatCov S = lpd_feat_cov(m, k);
    const LpdFeatEig e = lpd_feat_eig(S);
    const float s = e.l1 + e.l2 + e.l3;
    f[0] = f[1] = f[2] = f[3] = f[4] = 0.0f;
    if (s > 0.0f) {
        const float e1 = e.l1 / s, e2 = e.l2 / s, e3 = e.l3 / s;
        f[0] = e3;                                                             // change of curvature
        f[1] = cbrtf(e1 * e2 * e3);                                            // omnivariance
        f[2] = e.l1 > 0.0f ? (e.l1 - e.l2) / e.l1 : 0.0f;                      // linearity
        f[3] = lpd_feat_entropy(e);                                            // eigenentropy (the value the adaptive size minimises)
        f[4] = fabsf(e.nz);                                                    // vertical component of the normal
    }
    f[5] = S.xx + S.yy;                                                        // 2-D scattering
    // 2-D linearity: eigenvalues of the xy block, closed form h +- d
    const float h = 0.5f * (S.xx + S.yy), g = 0.5f * (S.xx - S.yy);
    const float d = sqrtf(g * g + S.xy * S.xy);
    const float big = h + d, small = fmaxf(h - d, 0.0f);
    f[6] = big > 0.0f ? small / big : 0.0f;
    f[7] = m.zmax - m.zmin;                                                    // height range
    f[8] = S.zz;                                                               // height variance
    const float r = sqrtf(m.r2);
    const float vol = 4.18879020478639f * (r * r * r);                         // (4/3) pi r^3
    f[9] = vol > 0.0f ? fminf((float)k / vol, FLT_MAX) : 0.0f;                 // local point density
}
