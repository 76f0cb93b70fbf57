// Density normals (header section 12): the gradient of the raw density with respect to the multisample positions, per sample, its
// negative normalised, and that composited along the ray (ZI/models.py:1075-1094 with analytic_gradient, render.py:255-261).
//
//   f   = the features of nlr_encode_features_forward                     [N*S, F], F = L*C
//   g_f = W0^T (1[W0 f + b0 > 0] . w2_row0)                               the cotangent of raw_density = density_layer(f)[..., 0]
//   G   = (1/n) sum_j gm_j,  gm_j = nlr_multisample_adjoint(g_f)          the reference's autograd.grad(...).mean(-2)
//   nrm = -G / max(|G|, 1e-5),  ray_normals = sum_s weights_s nrm_s
//
// Three launches: the feature pass (the inference path's kernel, called, not restated), (a) nlr_density_cotangent_kernel and (b)
// nlr_sample_normals_kernel, a sibling of nlr_encode_rays_kernel that reduces the same per-multisample adjoint per SAMPLE.  No
// atomics: a sample's sum runs over j ascending in one lane, a ray's over s ascending by 64 in each lane and then an xor butterfly,
// so every output is bitwise repeatable and does not depend on the launch.
#include "nlr_kernels.h"

#include "nlr_encode_adjoint.h"

#define NLR_NORMALS_HIDDEN 64u
#define NLR_NORMALS_FMAX 64u
#define NLR_RAYS_PER_BLOCK 4u

static inline size_t nlr_normals_ws_bytes(uint32_t N, uint32_t S, uint32_t F) { return (size_t)2 * N * S * F * sizeof(float); }

// (a) One lane per sample, density_layer.0 and row 0 of density_layer.2 in LDS (64 F + 128 floats: 16.5 KiB at F = 64), the sample's
// features in registers.  Per hidden unit h, ascending: a_h = b0_h + sum_i w0[h][i] f_i (i ascending), then g_f += [a_h > 0] w2_h w0[h][:].
// FP = F rounded up to a multiple of 16: the register arrays' size; the guards `q < F / 4` are wave-uniform.
template <int FP>
__global__ void __launch_bounds__(256) nlr_density_cotangent_kernel(const float *__restrict__ feat, const float *__restrict__ w0,
                                                                    const float *__restrict__ b0, const float *__restrict__ w2, uint32_t M,
                                                                    uint32_t F, float *__restrict__ g_feat) {
    __shared__ float4 sw4[(NLR_NORMALS_HIDDEN * FP + 2 * NLR_NORMALS_HIDDEN) / 4];  // w0 [64][F] | b0 [64] | w2 [64]
    float *sw = (float *)sw4;
    for (uint32_t i = threadIdx.x; i < NLR_NORMALS_HIDDEN * F; i += blockDim.x) sw[i] = w0[i];
    if (threadIdx.x < NLR_NORMALS_HIDDEN) {
        sw[NLR_NORMALS_HIDDEN * F + threadIdx.x] = b0[threadIdx.x];
        sw[NLR_NORMALS_HIDDEN * F + NLR_NORMALS_HIDDEN + threadIdx.x] = w2[threadIdx.x];
    }
    __syncthreads();
    const uint32_t Q = F / 4;
    for (uint32_t m = blockIdx.x * blockDim.x + threadIdx.x; m < M; m += gridDim.x * blockDim.x) {
        float4 f[FP / 4], df[FP / 4];
        const float4 *row = (const float4 *)(feat + (size_t)m * F);  // F % 4 == 0 and the buffer is 16-byte aligned (checked by the launcher)
#pragma unroll
        for (int q = 0; q < FP / 4; ++q) {
            f[q] = (uint32_t)q < Q ? row[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            df[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        for (uint32_t h = 0; h < NLR_NORMALS_HIDDEN; ++h) {
            const float4 *wr = (const float4 *)(sw + h * F);
            float a = sw[NLR_NORMALS_HIDDEN * F + h];
#pragma unroll
            for (int q = 0; q < FP / 4; ++q)
                if ((uint32_t)q < Q) {
                    const float4 w = wr[q];
                    a = fmaf(w.x, f[q].x, a), a = fmaf(w.y, f[q].y, a), a = fmaf(w.z, f[q].z, a), a = fmaf(w.w, f[q].w, a);
                }
            const float dh = a > 0.0f ? sw[NLR_NORMALS_HIDDEN * F + NLR_NORMALS_HIDDEN + h] : 0.0f;
#pragma unroll
            for (int q = 0; q < FP / 4; ++q)
                if ((uint32_t)q < Q) {
                    const float4 w = wr[q];
                    df[q].x = fmaf(dh, w.x, df[q].x), df[q].y = fmaf(dh, w.y, df[q].y), df[q].z = fmaf(dh, w.z, df[q].z), df[q].w = fmaf(dh, w.w, df[q].w);
                }
        }
        float4 *out = (float4 *)(g_feat + (size_t)m * F);
#pragma unroll
        for (int q = 0; q < FP / 4; ++q)
            if ((uint32_t)q < Q) out[q] = df[q];
    }
}

// (b) One wave per ray.  Lane i owns the samples i, i + 64, ...: for each it walks the multisamples j = 0..n-1 and all levels of each
// (8 * C gathers in flight per level), averages, normalises and stores; its share of sum_s weights_s nrm_s stays in registers and an
// xor butterfly over the 64 lanes sums the shares (idle lanes hold 0) before lane 0 stores the ray's normal.
template <typename T, int C>
__global__ void __launch_bounds__(256) nlr_sample_normals_kernel(CastParams cp, GridParams gp, int re_weights, const float *__restrict__ g_feat,
                                                                 const float *__restrict__ weights, float *__restrict__ raw_grad,
                                                                 float *__restrict__ normals, float *__restrict__ ray_normals) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t ray = blockIdx.x * NLR_RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= cp.N) return;  // (a whole wave, before any cross-lane operation: the kernel has no barrier)
    RayRegs rr = nlr_load_ray(cp, ray);
    const float inv_n = 1.0f / (float)cp.n;
    const uint32_t LC = gp.L * C;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (uint32_t k = lane; k < cp.S; k += 64u) {
        nlr_load_span(cp, ray, k, rr);
        const size_t row = (size_t)ray * cp.S + k;
        const float *gf = g_feat + row * LC;
        float G[3] = {0.0f, 0.0f, 0.0f};
        for (uint32_t j = 0; j < cp.n; ++j) {
            CastTaps tp;
            float gm[3];
            if (!nlr_multisample_adjoint<T, C>(cp, gp, re_weights, ray, k, j, rr, gf, inv_n, tp, gm)) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) G[c] += gm[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) G[c] = G[c] / (float)cp.n;  // .mean(-2) (models.py:1089)
        // -F.normalize(G, eps = 1e-5) (ref_utils.py:23-25, models.py:1094): a zero gradient gives a zero normal
        const float len = fmaxf(sqrtf((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]), 1e-5f);
        float nrm[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) nrm[c] = -(G[c] / len);
        if (raw_grad) {
#pragma unroll
            for (int c = 0; c < 3; ++c) raw_grad[row * 3 + c] = G[c];
        }
        if (normals) {
#pragma unroll
            for (int c = 0; c < 3; ++c) normals[row * 3 + c] = nrm[c];
        }
        if (ray_normals) {
            const float w = weights[row];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = fmaf(w, nrm[c], acc[c]);
        }
    }
    if (!ray_normals) return;  // (kernel argument: the whole wave)
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = nlr_wave_sum(acc[c]);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) ray_normals[(size_t)ray * 3 + c] = acc[c];
    }
}

extern "C" size_t nlr_density_normals_workspace_bytes(uint32_t N, uint32_t S, uint32_t F) { return nlr_normals_ws_bytes(N, S, F); }

extern "C" int nlr_density_normals(const NlrRays *rays, const float *tdist, uint32_t N, uint32_t S, uint32_t sample_n, uint32_t sample_m,
                                   float std_scale, const float *rand_deg, const NlrGridDesc *grid, uint32_t re_weights, uint32_t hidden,
                                   const float *w0, const float *b0, const float *w2_row0, const float *weights, float *raw_grad,
                                   float *normals, float *ray_normals, void *workspace, size_t workspace_bytes, void *stream) {
    if (N == 0) return NLR_OK;
    NLR_CHECK_ARG(grid && grid->table && grid->offsets && tdist && w0 && b0 && w2_row0, "density_normals: NULL argument");
    NLR_CHECK_ARG(S >= 1, "density_normals: S = 0 samples");
    NLR_CHECK_ARG(!ray_normals || weights, "density_normals: ray_normals needs weights");
    if (grid->level_dim != 1 && grid->level_dim != 2 && grid->level_dim != 4 && grid->level_dim != 8)
        NLR_FAIL(NLR_ERR_UNSUPPORTED, "density_normals: level_dim = %u, the kernel has instances for 1, 2, 4 and 8", grid->level_dim);
    if (grid->table_dtype != 0 && grid->table_dtype != 1)
        NLR_FAIL(NLR_ERR_UNSUPPORTED, "density_normals: table_dtype = %d, the kernel reads f32 (0) and f16 (1) tables", (int)grid->table_dtype);
    const uint32_t F = grid->num_levels * grid->level_dim;
    if (F == 0 || F > NLR_NORMALS_FMAX || F % 4 != 0)
        NLR_FAIL(NLR_ERR_UNSUPPORTED, "density_normals: F = L * C = %u features, the cotangent kernel takes a multiple of 4 up to %u", F,
                 NLR_NORMALS_FMAX);
    if (hidden != NLR_NORMALS_HIDDEN)
        NLR_FAIL(NLR_ERR_UNSUPPORTED, "density_normals: hidden width %u of density_layer.0, the cotangent kernel is built for %u", hidden,
                 NLR_NORMALS_HIDDEN);
    const size_t need = nlr_normals_ws_bytes(N, S, F);
    if (!workspace || workspace_bytes < need)
        NLR_FAIL(NLR_ERR_WORKSPACE, "density_normals: workspace %s, %zu bytes given, nlr_density_normals_workspace_bytes(%u, %u, %u) = %zu",
                 workspace ? "too small" : "is NULL", workspace ? workspace_bytes : (size_t)0, N, S, F, need);
    NLR_CHECK_ARG(((uintptr_t)workspace & 15u) == 0, "density_normals: the workspace must be 16-byte aligned");
    CastParams cp;
    GridParams gp;
    int rc = nlr_encode_features_args(&cp, &gp, rays, tdist, N, S, sample_n, sample_m, std_scale, rand_deg, grid);
    if (rc) return rc;
    NLR_CHECK_ARG((uint64_t)S + 64 < (1ull << 32), "density_normals: S = %u does not fit the 32-bit sample counter", S);
    const uint64_t M = (uint64_t)N * S;
    NLR_CHECK_ARG(M + 256ull * 4096 < (1ull << 32), "density_normals: N * S = %llu samples do not fit the 32-bit sample index (chunk the rays)",
                  (unsigned long long)M);
    hipStream_t st = (hipStream_t)stream;
    float *feat = (float *)workspace, *g_feat = feat + (size_t)M * F;  // [N*S, F] each; N*S*F*4 is a multiple of 16
    rc = nlr_launch_encode(cp, gp, (int)re_weights, feat, 0, st);
    if (rc) return rc;
    const uint32_t blocks = (uint32_t)((M + 255) / 256);
    const dim3 cgrid(blocks < 4096 ? blocks : 4096), block(256);
    const uint32_t fp = (F + 15) / 16;
#define NLR_COT(FP)                                                                                                              \
    hipLaunchKernelGGL((nlr_density_cotangent_kernel<FP>), cgrid, block, 0, st, (const float *)feat, w0, b0, w2_row0, (uint32_t)M, F, g_feat)
    if (fp == 1) NLR_COT(16);
    else if (fp == 2) NLR_COT(32);
    else if (fp == 3) NLR_COT(48);
    else NLR_COT(64);
#undef NLR_COT
    NLR_LAUNCH_CHECK("nlr_density_cotangent_kernel");
    if (!raw_grad && !normals && !ray_normals) return NLR_OK;
    const dim3 ngrid((N + NLR_RAYS_PER_BLOCK - 1) / NLR_RAYS_PER_BLOCK), nblock(64 * NLR_RAYS_PER_BLOCK);
    nlr_dispatch_tc(gp, [&](auto t, auto c) {
        hipLaunchKernelGGL((nlr_sample_normals_kernel<decltype(t), decltype(c)::value>), ngrid, nblock, 0, st, cp, gp, (int)re_weights,
                           (const float *)g_feat, weights, raw_grad, normals, ray_normals);
    });
    NLR_LAUNCH_CHECK("nlr_sample_normals_kernel");
    return NLR_OK;
}
