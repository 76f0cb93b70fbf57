// One multisample of one interval: cone casting (render.py:129-168), contraction (coord.py:51-63) and the map to the unit cube, and
// the erf down-weighting of its level features (models.py:976).  Shared by the fused cast + encode kernels (nlr_encode.hip) and the
// ray gradient of that operator (nlr_encode_rays.hip), so the forward map is stated once.
#pragma once
#include "nlr_grid_level.h"

// What the ray gradient needs of the forward besides the Gauss: m = o + t d + lx bx + ly by BEFORE the contraction, its clamped
// squared norm, the footprint before the contraction, and which branch of the contraction ran.
struct CastTaps {
    float t, lx, ly, p[3], m2, std;
    bool contracted;
};

// What a kernel holds of a ray and of the interval [t0, t1] of its tdist row it works on: nlr_load_ray fills the first part, nlr_load_span
// the second (a kernel that walks a ray's samples loads the ray once and the interval per sample).
struct RayRegs {
    float o[3], d[3], bx[3], by[3], radius, t0, t1;
};
__device__ __forceinline__ RayRegs nlr_load_ray(const CastParams &cp, uint32_t ray) {
    RayRegs r;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        r.o[c] = cp.origins[(size_t)ray * 3 + c];
        r.d[c] = cp.directions[(size_t)ray * 3 + c];
        r.bx[c] = cp.base_x[(size_t)ray * 3 + c];
        r.by[c] = cp.base_y[(size_t)ray * 3 + c];
    }
    r.radius = cp.radii[ray];
    return r;
}
__device__ __forceinline__ void nlr_load_span(const CastParams &cp, uint32_t ray, uint32_t k, RayRegs &r) {
    r.t0 = cp.tdist[(size_t)ray * (cp.S + 1) + k];
    r.t1 = cp.tdist[(size_t)ray * (cp.S + 1) + k + 1];
}
__device__ __forceinline__ RayRegs nlr_load_ray(const CastParams &cp, uint32_t ray, uint32_t k) {
    RayRegs r = nlr_load_ray(cp, ray);
    nlr_load_span(cp, ray, k, r);
    return r;
}

__device__ __forceinline__ Gauss nlr_cast_one(const CastParams &cp, uint32_t ray, uint32_t k, uint32_t j, float t0, float t1,
                                              const float *o, const float *d, const float *bx, const float *by, float radius,
                                              float *raw = nullptr, CastTaps *taps = nullptr) {
    // render.py:147-156
    const float t = t0 + ((t1 - t0) * ((float)j + 0.5f)) / (float)cp.n;
    float cd = cp.cosd[j], sd = cp.sind[j];
    if (cp.rand_deg) {
        const float u = cp.rand_deg[((size_t)ray * cp.S + k) * cp.n + j];
        const float deg = cp.degj[j] + (u * 3.14159274101257324f) * 2.0f;
        cd = cosf(deg);
        sd = sinf(deg);
    }
    const float lx = ((radius * t) * cd) / 2.0f;
    const float ly = ((radius * t) * sd) / 2.0f;
    float m[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) m[c] = fmaf(t, d[c], fmaf(ly, by[c], lx * bx[c])) + o[c];  // render.py:162-164
    const float std = (cp.std_scale * radius) * t;
    // coord.py:51-63
    const float m2 = fmaxf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2], NLR_EPS);
    if (taps) {
        taps->t = t, taps->lx = lx, taps->ly = ly, taps->m2 = m2, taps->std = std;
        taps->p[0] = m[0], taps->p[1] = m[1], taps->p[2] = m[2];
        taps->contracted = !(m2 <= 1.0f);
    }
    float zs = std;
    if (!(m2 <= 1.0f)) {
        const float sq = sqrtf(m2);
        const float sc = (2.0f * sq - 1.0f) / m2;
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = sc * m[c];
        const float a = 2.0f / sq - 1.0f / m2;
        const float det = (1.0f / m2) * (a * a);
        // det ** (1/3) (coord.py:61).  cbrtf (17 VALU instructions) instead of powf(det, 0.33333334f) (164): the two differ by
        // det^(1e-8), i.e. <= 2 ulp, in a value that only scales the erf re-weighting argument
        zs = cbrtf(det) * std;
    }
    Gauss g;
    // models.py:971-973 (bound = 2) then grid.py:162 ((x + 1) / 2)
    g.x0 = (m[0] / 2.0f + 1.0f) / 2.0f;
    g.x1 = (m[1] / 2.0f + 1.0f) / 2.0f;
    g.x2 = (m[2] / 2.0f + 1.0f) / 2.0f;
    g.zs = zs / 2.0f;
    if (raw) {  // means / bound as GridEncoder(bound=1) takes them (models.py:969-973)
        raw[0] = m[0] / 2.0f;
        raw[1] = m[1] / 2.0f;
        raw[2] = m[2] / 2.0f;
    }
    return g;
}
__device__ __forceinline__ Gauss nlr_cast_one(const CastParams &cp, uint32_t ray, uint32_t k, uint32_t j, const RayRegs &rr, float *raw = nullptr,
                                              CastTaps *taps = nullptr) {
    return nlr_cast_one(cp, ray, k, j, rr.t0, rr.t1, rr.o, rr.d, rr.bx, rr.by, rr.radius, raw, taps);
}

// models.py:976: erf(1 / clamp(sqrt(8 * std^2 * G^2), min=1e-10))
__device__ __forceinline__ float nlr_erf_weight(float zs, float gsize) {
    return erff(1.0f / fmaxf(sqrtf((8.0f * (zs * zs)) * (gsize * gsize)), 1e-10f));
}
// The same weight with the level-independent part hoisted: 1/sqrt(8 std^2 G^2) = inv_s8 / G with
// inv_s8 = 1/sqrt(8 std^2) computed once per multisample (differs from the reference's rounding order by a few
// ulp of the erf ARGUMENT, i.e. <= 3e-7 of the weight; the clamp at 1e-10 maps to an argument cap of 1e10).
__device__ __forceinline__ float nlr_erf_weight_fast(float inv_s8, float inv_g) {
    return erff(fminf(inv_s8 * inv_g, 1e10f));
}

// ---- host: kernel instance for a grid ------------------------------------------------------------------------------------------
template <int V>
struct NlrInt {
    static constexpr int value = V;
};
// f(T{}, NlrInt<C>{}) with T the table's element type and C the features per level; a C outside {1, 2, 4} takes the 8-wide instance.
template <typename F>
static inline void nlr_dispatch_tc(const GridParams &gp, F &&f) {
    auto with_c = [&](auto t) {
        switch (gp.C) {
            case 1: f(t, NlrInt<1>{}); break;
            case 2: f(t, NlrInt<2>{}); break;
            case 4: f(t, NlrInt<4>{}); break;
            default: f(t, NlrInt<8>{}); break;
        }
    };
    if (gp.table_dtype == 0) with_c(float{});
    else with_c(__half{});
}
