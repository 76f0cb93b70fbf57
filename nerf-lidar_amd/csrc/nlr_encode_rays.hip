// Ray gradient of the fused cast + encode operator (header section 9): d loss / d (origins, directions, base_x, base_y) from the
// gradient of the features, for pose refinement (ZI/train.py:199-221: the refined pose moves exactly these tensors).
//
// With m = o + t d + lx bx + ly by (t, lx, ly, std: functions of tdist, radii, rand_deg - data) the four outputs are sum gm, sum t gm,
// sum lx gm, sum ly gm of the per-multisample adjoint gm = d loss / d m, which nlr_encode_adjoint.h states (shared with the density
// normals, nlr_normals.hip).
//
// One wave per ray.  Lane i walks the ray's (sample, multisample) pairs i, i + 64, ... and all levels of each, 8 * C gathers in flight
// per level, and keeps the ray's 12 numbers in registers; an xor butterfly over the 64 lanes then sums them and lane 0 stores.  No
// atomics: the order of every sum is fixed by (S, n, L) alone, so the result is bitwise repeatable and does not depend on the launch.
#include "nlr_kernels.h"

#include "nlr_encode_adjoint.h"

#define NLR_RAYS_PER_BLOCK 4u

template <typename T, int C>
__global__ void __launch_bounds__(256) nlr_encode_rays_kernel(CastParams cp, GridParams gp, int re_weights, const float *__restrict__ d_feat,
                                                              float *__restrict__ d_o, float *__restrict__ d_d, float *__restrict__ d_bx,
                                                              float *__restrict__ d_by) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t ray = blockIdx.x * NLR_RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= cp.N) return;  // (a whole wave: the kernel has no barrier)
    RayRegs rr = nlr_load_ray(cp, ray);
    const float inv_n = 1.0f / (float)cp.n;
    const uint32_t LC = gp.L * C;
    float acc[12];  // d_o | d_d | d_bx | d_by
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 0.0f;
    const uint32_t items = cp.S * cp.n;
    for (uint32_t it = lane; it < items; it += 64u) {
        const uint32_t k = it / cp.n, j = it - k * cp.n;
        CastTaps tp;
        nlr_load_span(cp, ray, k, rr);
        float gm[3];
        if (!nlr_multisample_adjoint<T, C>(cp, gp, re_weights, ray, k, j, rr, d_feat + ((size_t)ray * cp.S + k) * LC, inv_n, tp, gm))
            continue;  // outside the unit cube: encodes as zeros on every level, no gradient
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            acc[c] += gm[c];
            acc[3 + c] = fmaf(tp.t, gm[c], acc[3 + c]);
            acc[6 + c] = fmaf(tp.lx, gm[c], acc[6 + c]);
            acc[9 + c] = fmaf(tp.ly, gm[c], acc[9 + c]);
        }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = nlr_wave_sum(acc[i]);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (d_o) d_o[(size_t)ray * 3 + c] = acc[c];
            if (d_d) d_d[(size_t)ray * 3 + c] = acc[3 + c];
            if (d_bx) d_bx[(size_t)ray * 3 + c] = acc[6 + c];
            if (d_by) d_by[(size_t)ray * 3 + c] = acc[9 + c];
        }
    }
}

extern "C" int nlr_encode_features_backward_rays(const NlrRays *rays, const float *tdist, uint32_t N, uint32_t S, uint32_t sample_n,
                                                 uint32_t sample_m, float std_scale, const float *rand_deg, const NlrGridDesc *grid,
                                                 uint32_t re_weights, const float *d_features, float *d_origins, float *d_directions,
                                                 float *d_base_x, float *d_base_y, void *stream) {
    if (N == 0) return NLR_OK;
    NLR_CHECK_ARG(grid && grid->table && grid->offsets && tdist && d_features, "encode_features_backward_rays: NULL argument");
    if (grid->level_dim != 1 && grid->level_dim != 2 && grid->level_dim != 4 && grid->level_dim != 8)
        NLR_FAIL(NLR_ERR_UNSUPPORTED, "encode_features_backward_rays: level_dim = %u, the kernel has instances for 1, 2, 4 and 8", grid->level_dim);
    if (grid->table_dtype != 0 && grid->table_dtype != 1)
        NLR_FAIL(NLR_ERR_UNSUPPORTED, "encode_features_backward_rays: table_dtype = %d, the kernel reads f32 (0) and f16 (1) tables",
                 (int)grid->table_dtype);
    CastParams cp;
    GridParams gp;
    int rc = nlr_encode_features_args(&cp, &gp, rays, tdist, N, S, sample_n, sample_m, std_scale, rand_deg, grid);
    if (rc) return rc;
    // (a lane's pair counter advances by 64 past the last pair before it stops)
    NLR_CHECK_ARG((uint64_t)S * sample_n + 64 < (1ull << 32), "encode_features_backward_rays: S * sample_n = %llu does not fit the 32-bit pair counter",
                  (unsigned long long)S * sample_n);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid_dim((N + NLR_RAYS_PER_BLOCK - 1) / NLR_RAYS_PER_BLOCK), block(64 * NLR_RAYS_PER_BLOCK);
    nlr_dispatch_tc(gp, [&](auto t, auto c) {
        hipLaunchKernelGGL((nlr_encode_rays_kernel<decltype(t), decltype(c)::value>), grid_dim, block, 0, st, cp, gp, (int)re_weights, d_features,
                           d_origins, d_directions, d_base_x, d_base_y);
    });
    NLR_LAUNCH_CHECK("nlr_encode_rays_kernel");
    return NLR_OK;
}
