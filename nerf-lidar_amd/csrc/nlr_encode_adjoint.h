// The adjoint of ONE multisample of the fused cast + encode operator: gm = d (sum_l g_l . f_l) / d m, m = o + t d + lx bx + ly by the
// multisample position of render.py:147-164 BEFORE the contraction.  Stated once, for the two kernels that reduce it differently:
// nlr_encode_rays_kernel (nlr_encode_rays.hip: per ray, for pose refinement) and nlr_sample_normals_kernel (nlr_normals.hip: per
// sample, the density gradient behind the surface normals).
//
// The forward map is nlr_cast_one + nlr_erf_weight_fast + the trilinear gather of nlr_grid_level.h:
//   y = m or contract(m),  zs = std or cbrt(det J) std      (coord.py:51-63; the branch is m2 > 1)
//   x01 = (y / 2 + 1) / 2,  f_l = (1/n) sum_j w_l(zs_j) tri_l(x01_j)
// and per multisample and level, with upstream g_l, the chain is
//   g_l . [ w_l dtri_l/dx dx/dm + tri_l dw_l/dzs dzs/dm ]
// (second term only with re_weights on a contracted sample).  At a cell face, at m2 = 1 and at the clamp of the erf argument the
// derivative is that of the branch the forward takes.
#pragma once
#include "nlr_cast.h"
#include "nlr_grid_level.h"

// gf: the upstream gradient of the sample's features [L*C]; inv_n = 1 / n, the weight of a multisample in the feature mean.  The caller
// has loaded the interval (nlr_load_span).  Returns false, with gm untouched, for a point outside the unit cube: it encodes as zeros
// on every level and carries no gradient.  `tp` receives the taps of the cast (t, lx, ly for the ray tensors' shares).
template <typename T, int C>
__device__ __forceinline__ bool nlr_multisample_adjoint(const CastParams &cp, const GridParams &gp, int re_weights, uint32_t ray, uint32_t k,
                                                        uint32_t j, const RayRegs &rr, const float *__restrict__ gf, float inv_n, CastTaps &tp,
                                                        float (&gm)[3]) {
    const Gauss g = nlr_cast_one(cp, ray, k, j, rr, nullptr, &tp);
    if (nlr_outside_unit_cube(g)) return false;
    const float inv_s8 = __frsqrt_rn(8.0f * (g.zs * g.zs));
    const bool footprint = re_weights && tp.contracted;  // zs depends on the position only through the contraction
    float gx[3] = {0.0f, 0.0f, 0.0f}, gzs = 0.0f;  // d / d x01, d / d g.zs of this multisample's share of the loss
    for (uint32_t l = 0; l < gp.L; ++l) {
        float up[C];
#pragma unroll
        for (int c = 0; c < C; ++c) up[c] = gf[l * C + c] * inv_n;
        float dp[3], tri;
        nlr_level_grad<T, C>(gp, l, g, up, dp, tri);
        float w = 1.0f;
        if (re_weights) {
            const float u = inv_s8 * gp.inv_gsize[l];  // nlr_erf_weight_fast: w = erf(min(u, 1e10)), u = 1 / (sqrt(8) zs G)
            w = erff(fminf(u, 1e10f));
            // dw/dzs = 2/sqrt(pi) exp(-u^2) du/dzs, du/dzs = -u / zs; nothing beyond the cap
            if (footprint && u < 1e10f) gzs = fmaf(tri, (1.1283791670955126f * expf(-(u * u))) * (-u / g.zs), gzs);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) gx[c] = fmaf(w, dp[c], gx[c]);
    }
    // x01 = (y / 2 + 1) / 2, g.zs = zs / 2
    gm[0] = gx[0] * 0.25f, gm[1] = gx[1] * 0.25f, gm[2] = gx[2] * 0.25f;
    if (tp.contracted) {
        // y = sc(m2) p, sc = (2 sqrt(m2) - 1) / m2; zs = cbrt(det) std, det = sc^2 / m2; m2 = |p|^2 (its clamp at eps is far below 1)
        const float m2 = tp.m2, sq = sqrtf(m2);
        const float sc = (2.0f * sq - 1.0f) / m2;
        const float dsc = (1.0f / m2 - 1.0f / sq) / m2;  // d sc / d m2 = m2^-2 - m2^-3/2
        const float gy_p = (gm[0] * tp.p[0] + gm[1] * tp.p[1]) + gm[2] * tp.p[2];
        float along = gy_p * dsc;  // coefficient of d m2 / d p = 2 p
        if (footprint) {
            // d zs / d m2 = zs / (3 det) d det / d m2, d det / d m2 = (2 sc dsc - sc^2 / m2) / m2
            const float det = (1.0f / m2) * (sc * sc);
            const float ddet = (2.0f * sc * dsc - (sc * sc) / m2) / m2;
            const float zs = cbrtf(det) * tp.std;
            along = fmaf(gzs * 0.5f, (zs / (3.0f * det)) * ddet, along);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) gm[c] = fmaf(2.0f * along, tp.p[c], sc * gm[c]);
    }
    return true;
}
