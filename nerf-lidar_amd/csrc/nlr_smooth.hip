// Edge-aware smoothness of the rendered depth and class probabilities over pixel patches: the two terms the reference puts on its
// patch rays (ZI/train.py:365-388; train_utils.py:330-348 edge_aware_loss_v2, :411-433 edge_aware_loss_for_semantic, both on their
// `mask is not None` branch).
//
// A batch is P patches of s x s pixels, row (p*s + i)*s + j = pixel (i, j) of patch p; "x" neighbours differ in j, "y" in i.
// A channel is the depth (channel 0, eps 1e-7) or one class of the semantic input (channels 1..K, eps 1e-5).  Per patch a channel is
// divided by (its mean over the patch + eps); a pair of neighbours contributes |D - D'| * exp(-mean_c |rgb - rgb'|) when both
// pixels are valid; each term is sum_x / #x-pairs + sum_y / #y-pairs over ALL patches (the reference takes one mean over the
// selected pairs of the batch), and 0 with zero gradient when either count is 0 (its nan_to_num of a mean of nothing).
//
// One workgroup per (patch, slice of NLR_SMOOTH_CPS channels).  The pair weights (validity folded in: 0 = no pair) are computed once
// per workgroup into LDS, the normalised channel is staged in LDS, the workgroup loops over its channels.  Per-workgroup sums and
// per-patch counts go to the workspace, a one-wave kernel adds them in a fixed order: no atomics, same inputs -> same bits.
// The backward recomputes means and differences from the inputs and reads the counts and the upstream scalars from device memory.
#include "nlr_common.h"

#define NLR_SMOOTH_CPS 4       // channels per workgroup
#define NLR_SMOOTH_THREADS 256
#define NLR_SMOOTH_MAX_S 64
#define NLR_SMOOTH_MAX_K 32

static inline uint32_t nlr_smooth_slices(uint32_t K) { return (1 + K + NLR_SMOOTH_CPS - 1) / NLR_SMOOTH_CPS; }
// workspace: float part[P * slices * 4] (depth x, depth y, semantic x, semantic y), then uint32 cnt[P * 2] (x pairs, y pairs)
static inline size_t nlr_smooth_ws_bytes(uint32_t P, uint32_t K) { return ((size_t)P * nlr_smooth_slices(K) * 4 + (size_t)P * 2) * 4; }

extern "C" size_t nlr_patch_smooth_workspace_bytes(uint32_t P, uint32_t K) { return nlr_smooth_ws_bytes(P, K); }

struct SmoothParams {
    const float *depth, *semantic, *rgb, *valid;
    uint32_t P, s, K, C;  // C = channels: 1 + K with a semantic input, else 1
};

// sum over the workgroup, the same value in every thread; waves first (xor tree), then the four wave sums in wave order
template <typename T>
__device__ __forceinline__ T nlr_smooth_block_sum(T v, T *red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();  // red may still be read from the previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T t = red[0];
#pragma unroll
    for (int w = 1; w < NLR_SMOOTH_THREADS / 64; ++w) t += red[w];
    return t;
}

// pair weights of the patch into LDS: wx[i*s + j] for the pair (i,j)-(i,j+1), wy[i*s + j] for (i,j)-(i+1,j); 0 where there is no
// such pair (last column / row) or one of its pixels is invalid.  nx, ny: this thread's pair counts.
__device__ __forceinline__ void nlr_smooth_weights(const SmoothParams &A, uint32_t p, float *wx, float *wy, uint32_t &nx, uint32_t &ny) {
    const uint32_t s = A.s, n = s * s;
    const size_t base = (size_t)p * n;
    nx = ny = 0;
    for (uint32_t q = threadIdx.x; q < n; q += NLR_SMOOTH_THREADS) {
        const uint32_t i = q / s, j = q - i * s;
        const float *c0 = A.rgb + (base + q) * 3;
        const bool v0 = !A.valid || A.valid[base + q] > 0.0f;
        float ex = 0.0f, ey = 0.0f;
        if (j + 1 < s && v0 && (!A.valid || A.valid[base + q + 1] > 0.0f)) {
            const float *c1 = c0 + 3;
            ex = expf(-((fabsf(c0[0] - c1[0]) + fabsf(c0[1] - c1[1]) + fabsf(c0[2] - c1[2])) / 3.0f));
            ++nx;
        }
        if (i + 1 < s && v0 && (!A.valid || A.valid[base + q + s] > 0.0f)) {
            const float *c1 = c0 + 3 * (size_t)s;
            ey = expf(-((fabsf(c0[0] - c1[0]) + fabsf(c0[1] - c1[1]) + fabsf(c0[2] - c1[2])) / 3.0f));
            ++ny;
        }
        wx[q] = ex;
        wy[q] = ey;
    }
}

// channel c of patch p, divided by (mean over the patch + eps), into LDS D[n]; returns mean + eps
__device__ __forceinline__ float nlr_smooth_stage(const SmoothParams &A, uint32_t p, uint32_t c, float *D, float *red) {
    const uint32_t n = A.s * A.s;
    const size_t base = (size_t)p * n;
    const float *src = c == 0 ? A.depth + base : A.semantic + base * A.K + (c - 1);
    const size_t stride = c == 0 ? 1 : A.K;
    float sum = 0.0f;
    for (uint32_t q = threadIdx.x; q < n; q += NLR_SMOOTH_THREADS) {
        const float x = src[q * stride];
        D[q] = x;
        sum += x;
    }
    const float denom = nlr_smooth_block_sum(sum, red) / (float)n + (c == 0 ? 1e-7f : 1e-5f);
    for (uint32_t q = threadIdx.x; q < n; q += NLR_SMOOTH_THREADS) D[q] = D[q] / denom;  // own elements only
    __syncthreads();
    return denom;
}

__global__ void __launch_bounds__(NLR_SMOOTH_THREADS) nlr_patch_smooth_fwd_kernel(SmoothParams A, float *__restrict__ part,
                                                                                 uint32_t *__restrict__ cnt) {
    extern __shared__ float lds[];
    __shared__ float red[NLR_SMOOTH_THREADS / 64];
    __shared__ uint32_t redu[NLR_SMOOTH_THREADS / 64];
    const uint32_t s = A.s, n = s * s, p = blockIdx.x, slice = blockIdx.y;
    float *wx = lds, *wy = lds + n, *D = lds + 2 * n;
    uint32_t nx, ny;
    nlr_smooth_weights(A, p, wx, wy, nx, ny);
    if (slice == 0) {
        nx = nlr_smooth_block_sum(nx, redu);
        ny = nlr_smooth_block_sum(ny, redu);
        if (threadIdx.x == 0) {
            cnt[(size_t)p * 2] = nx;
            cnt[(size_t)p * 2 + 1] = ny;
        }
    }
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // depth x, depth y, semantic x, semantic y
    const uint32_t c1 = min(A.C, (slice + 1) * NLR_SMOOTH_CPS);
    for (uint32_t c = slice * NLR_SMOOTH_CPS; c < c1; ++c) {
        nlr_smooth_stage(A, p, c, D, red);  // (its first barrier also orders the weights before the first read)
        float ax = 0.0f, ay = 0.0f;
        for (uint32_t q = threadIdx.x; q < n; q += NLR_SMOOTH_THREADS) {
            const uint32_t i = q / s, j = q - i * s;
            const float d = D[q];
            if (j + 1 < s) ax += fabsf(d - D[q + 1]) * wx[q];
            if (i + 1 < s) ay += fabsf(d - D[q + s]) * wy[q];
        }
        acc[c == 0 ? 0 : 2] += ax;
        acc[c == 0 ? 1 : 3] += ay;
        __syncthreads();  // D is overwritten by the next channel
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float v = nlr_smooth_block_sum(acc[t], red);
        if (threadIdx.x == 0) part[((size_t)p * gridDim.y + slice) * 4 + t] = v;
    }
}

// one wave: stats[0..3] = the four sums, stats[4..5] = the pair counts, terms = T_d, T_s
__global__ void __launch_bounds__(64) nlr_patch_smooth_sum_kernel(const float *__restrict__ part, const uint32_t *__restrict__ cnt, uint32_t P,
                                                                  uint32_t slices, int has_sem, float *__restrict__ terms,
                                                                  float *__restrict__ stats) {
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    unsigned long long nx = 0, ny = 0;
    const size_t rows = (size_t)P * slices;
    for (size_t r = threadIdx.x; r < rows; r += 64)
#pragma unroll
        for (int t = 0; t < 4; ++t) a[t] += (double)part[r * 4 + t];
    for (uint32_t p = threadIdx.x; p < P; p += 64) {
        nx += cnt[(size_t)p * 2];
        ny += cnt[(size_t)p * 2 + 1];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int t = 0; t < 4; ++t) a[t] += __shfl_xor(a[t], d, 64);
        nx += __shfl_xor(nx, d, 64);
        ny += __shfl_xor(ny, d, 64);
    }
    if (threadIdx.x == 0) {
        const bool live = nx > 0 && ny > 0;
        for (int t = 0; t < 4; ++t) stats[t] = (float)a[t];
        stats[4] = (float)nx;
        stats[5] = (float)ny;
        stats[6] = stats[7] = 0.0f;
        terms[0] = live ? (float)(a[0] / (double)nx + a[1] / (double)ny) : 0.0f;
        terms[1] = live && has_sem ? (float)(a[2] / (double)nx + a[3] / (double)ny) : 0.0f;
    }
}

// cotangent of the normalised value at pixel q = (i, j): signed pair weights from up to four neighbours (sign(0) = 0)
__device__ __forceinline__ float nlr_smooth_cot(const float *D, const float *wx, const float *wy, uint32_t s, uint32_t q, uint32_t i, uint32_t j,
                                                float kx, float ky) {
    const float d = D[q];
    auto sgn = [](float x) { return (float)((x > 0.0f) - (x < 0.0f)); };
    float ax = 0.0f, ay = 0.0f;
    if (j + 1 < s) ax += sgn(d - D[q + 1]) * wx[q];
    if (j > 0) ax += sgn(d - D[q - 1]) * wx[q - 1];
    if (i + 1 < s) ay += sgn(d - D[q + s]) * wy[q];
    if (i > 0) ay += sgn(d - D[q - s]) * wy[q - s];
    return ax * kx + ay * ky;
}

__global__ void __launch_bounds__(NLR_SMOOTH_THREADS) nlr_patch_smooth_bwd_kernel(SmoothParams A, const float *__restrict__ stats,
                                                                                 const float *__restrict__ g_terms, float *__restrict__ d_depth,
                                                                                 float *__restrict__ d_semantic) {
    extern __shared__ float lds[];
    __shared__ float red[NLR_SMOOTH_THREADS / 64];
    const uint32_t s = A.s, n = s * s, p = blockIdx.x, slice = blockIdx.y;
    const size_t base = (size_t)p * n;
    float *wx = lds, *wy = lds + n, *D = lds + 2 * n;
    const float nx = stats[4], ny = stats[5];
    const bool live = nx > 0.0f && ny > 0.0f;
    uint32_t ux, uy;
    if (live) nlr_smooth_weights(A, p, wx, wy, ux, uy);
    const uint32_t c1 = min(A.C, (slice + 1) * NLR_SMOOTH_CPS);
    for (uint32_t c = slice * NLR_SMOOTH_CPS; c < c1; ++c) {
        float *dst = c == 0 ? d_depth + base : d_semantic + base * A.K + (c - 1);
        const size_t stride = c == 0 ? 1 : A.K;
        if (!live) {  // uniform over the grid: the term is 0 and so is its gradient
            for (uint32_t q = threadIdx.x; q < n; q += NLR_SMOOTH_THREADS) dst[q * stride] = 0.0f;
            continue;
        }
        const float g = g_terms[c == 0 ? 0 : 1];
        const float kx = g / nx, ky = g / ny;
        const float denom = nlr_smooth_stage(A, p, c, D, red);
        float dot = 0.0f;  // sum_j a_j D_j: the share of every pixel through the patch mean
        for (uint32_t q = threadIdx.x; q < n; q += NLR_SMOOTH_THREADS) {
            const uint32_t i = q / s, j = q - i * s;
            dot += nlr_smooth_cot(D, wx, wy, s, q, i, j, kx, ky) * D[q];
        }
        dot = nlr_smooth_block_sum(dot, red) / (float)n;
        for (uint32_t q = threadIdx.x; q < n; q += NLR_SMOOTH_THREADS) {
            const uint32_t i = q / s, j = q - i * s;
            dst[q * stride] = (nlr_smooth_cot(D, wx, wy, s, q, i, j, kx, ky) - dot) / denom;
        }
        __syncthreads();  // D is overwritten by the next channel
    }
}

static int nlr_smooth_check(const char *fn, const float *depth, const float *rgb, uint32_t P, uint32_t s, uint32_t K, const void *workspace,
                            size_t workspace_bytes) {
    NLR_CHECK_ARG(depth, "%s: depth is NULL", fn);
    NLR_CHECK_ARG(rgb, "%s: rgb is NULL", fn);
    NLR_CHECK_ARG(P >= 1, "%s: P = 0 patches", fn);
    NLR_CHECK_ARG(s >= 2 && s <= NLR_SMOOTH_MAX_S, "%s: s = %u outside [2, %d]", fn, s, NLR_SMOOTH_MAX_S);
    NLR_CHECK_ARG(K >= 1 && K <= NLR_SMOOTH_MAX_K, "%s: K = %u outside [1, %d]", fn, K, NLR_SMOOTH_MAX_K);
    NLR_CHECK_ARG(workspace, "%s: workspace is NULL", fn);
    NLR_CHECK_ARG(workspace_bytes >= nlr_smooth_ws_bytes(P, K), "%s: workspace_bytes = %zu, nlr_patch_smooth_workspace_bytes(%u, %u) = %zu", fn,
                  workspace_bytes, P, K, nlr_smooth_ws_bytes(P, K));
    return NLR_OK;
}

extern "C" int nlr_patch_smooth_forward(const float *depth, const float *semantic, const float *rgb, const float *valid, uint32_t P, uint32_t s,
                                        uint32_t K, float *terms, float *stats, void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "patch_smooth_forward";
    if (int rc = nlr_smooth_check(fn, depth, rgb, P, s, K, workspace, workspace_bytes)) return rc;
    NLR_CHECK_ARG(terms, "%s: terms is NULL", fn);
    NLR_CHECK_ARG(stats, "%s: stats is NULL", fn);
    hipStream_t st = (hipStream_t)stream;
    SmoothParams A = {depth, semantic, rgb, valid, P, s, K, semantic ? 1 + K : 1};
    const uint32_t slices = (A.C + NLR_SMOOTH_CPS - 1) / NLR_SMOOTH_CPS;  // <= nlr_smooth_slices(K): what the workspace was sized for
    float *part = (float *)workspace;
    uint32_t *cnt = (uint32_t *)(part + (size_t)P * slices * 4);
    hipLaunchKernelGGL(nlr_patch_smooth_fwd_kernel, dim3(P, slices), dim3(NLR_SMOOTH_THREADS), 3 * s * s * sizeof(float), st, A, part, cnt);
    NLR_LAUNCH_CHECK("nlr_patch_smooth_fwd_kernel");
    hipLaunchKernelGGL(nlr_patch_smooth_sum_kernel, dim3(1), dim3(64), 0, st, part, cnt, P, slices, semantic != nullptr, terms, stats);
    NLR_LAUNCH_CHECK("nlr_patch_smooth_sum_kernel");
    return NLR_OK;
}

extern "C" int nlr_patch_smooth_backward(const float *depth, const float *semantic, const float *rgb, const float *valid, uint32_t P, uint32_t s,
                                         uint32_t K, const float *stats, const float *g_terms, float *d_depth, float *d_semantic, void *workspace,
                                         size_t workspace_bytes, void *stream) {
    const char *fn = "patch_smooth_backward";
    if (int rc = nlr_smooth_check(fn, depth, rgb, P, s, K, workspace, workspace_bytes)) return rc;
    NLR_CHECK_ARG(stats, "%s: stats is NULL", fn);
    NLR_CHECK_ARG(g_terms, "%s: g_terms is NULL", fn);
    NLR_CHECK_ARG(d_depth, "%s: d_depth is NULL", fn);
    NLR_CHECK_ARG(!semantic == !d_semantic, "%s: semantic and d_semantic must both be given or both be NULL", fn);
    SmoothParams A = {depth, semantic, rgb, valid, P, s, K, semantic ? 1 + K : 1};
    const uint32_t slices = (A.C + NLR_SMOOTH_CPS - 1) / NLR_SMOOTH_CPS;
    hipLaunchKernelGGL(nlr_patch_smooth_bwd_kernel, dim3(P, slices), dim3(NLR_SMOOTH_THREADS), 3 * s * s * sizeof(float), (hipStream_t)stream, A,
                       stats, g_terms, d_depth, d_semantic);
    NLR_LAUNCH_CHECK("nlr_patch_smooth_bwd_kernel");
    return NLR_OK;
}
