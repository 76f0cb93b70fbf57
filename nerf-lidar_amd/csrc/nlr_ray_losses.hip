// The two losses that read the ray history (header section 11): the distortion loss of the final level (ZI/train_utils.py:175-181,
// stepfun.py:297-308) and the Zip-NeRF anti-aliased interlevel loss of every proposal level (train_utils.py:134-172, stepfun.py:425-433
// blur_stepfun, math.py:111-131 sorted_interp_quad), values and gradients with respect to the weights.  sdist is data.
//
// One wave per (ray, term); a workgroup IS one wave, so __syncthreads() orders its LDS traffic and nothing waits on another wave.  A
// workgroup walks NLR_RL_RPB consecutive rays of one term (blockIdx.y: 0 = distortion, 1 + i = proposal level i) and leaves one partial
// sum and one count in the workspace; a one-wave kernel per term adds them in index order: no atomics, same inputs -> same bits.
//
// Anti-aliased term of a ray: the final level's histogram (c [S+1], pdf = min(w / dc, 10)) blurred with a box of half-width r is a
// piecewise-linear function with the M = 2S + 2 knots c - r, c + r.  Both lists are sorted, so the merged position of a knot is its own
// index plus its rank in the other list (a binary search in LDS; c - r goes first among equals, equal knots carry equal values).  Then
// five scans over the knots, lane l owning the contiguous chunk [l * ceil(M / 64), ..), the sums carried in float64 like torch's CPU
// cumsum: slope = scan(jump), val = max(scan(dk slope), 0), cdf = scan(trapezoids), the running max of val and its reverse running min
// (what the reference's find_interval makes of an unsorted pdf, see losses._quad_cdf_at), and one bracket look-up per proposal edge.
// NaNs travel as on torch (clamps and extrema written as comparisons): a zero-width bin with w = 0 poisons exactly its ray.
// LDS per wave: 4 arrays of M floats + S_i + 1 cdf values (18.5 KB at S = S_i = 512, 2.3 KB at S = S_i = 64).
#include "nlr_common.h"

#define NLR_RL_RPB 16  // rays per workgroup (= per partial sum)

static inline uint32_t nlr_rl_blocks(uint32_t N) { return (N + NLR_RL_RPB - 1) / NLR_RL_RPB; }
// workspace: float part[(1 + n_prop) * blocks], then uint32 cnt[(1 + n_prop) * blocks]
static inline size_t nlr_rl_ws_bytes(uint32_t N, uint32_t n_prop) { return (size_t)(1 + n_prop) * nlr_rl_blocks(N) * 8; }

extern "C" size_t nlr_ray_losses_workspace_bytes(uint32_t N, uint32_t n_prop) { return nlr_rl_ws_bytes(N, n_prop); }

struct RayLossParams {
    const float *sdist, *weights;
    const float *psd[NLR_RAY_LOSSES_MAX_PROP], *pw[NLR_RAY_LOSSES_MAX_PROP];
    const uint8_t *pm[NLR_RAY_LOSSES_MAX_PROP];
    float *wt[NLR_RAY_LOSSES_MAX_PROP];   // w_target: written by the forward, read by the backward
    float *dpw[NLR_RAY_LOSSES_MAX_PROP];  // backward only
    float *dw;                            // backward only
    uint32_t pS[NLR_RAY_LOSSES_MAX_PROP];
    float r[NLR_RAY_LOSSES_MAX_PROP];
    uint32_t N, S, n_prop;
};

// the running extrema's operators; they keep a NaN from either side, as torch.cummax / cummin do
struct RlMax {
    static __device__ __forceinline__ float id() { return -INFINITY; }
    static __device__ __forceinline__ float op(float a, float b) { return (a > b || a != a) ? a : b; }
};
struct RlMin {
    static __device__ __forceinline__ float id() { return INFINITY; }
    static __device__ __forceinline__ float op(float a, float b) { return (a < b || a != a) ? a : b; }
};

// in-place inclusive scan of a[0..n) in LDS by one wave (REV: from the last element down).  Lane l scans its chunk, the chunk totals are
// scanned across the lanes, the prefix of the lanes before is applied.  Barriers before and after.
template <typename OP, bool REV>
__device__ __forceinline__ void nlr_rl_scan(float *a, uint32_t n, uint32_t lane) {
    const uint32_t per = (n + 63) / 64;
    const uint32_t i0 = min(n, lane * per), i1 = min(n, i0 + per);
    __syncthreads();
    float acc = OP::id();
    for (uint32_t i = i0; i < i1; ++i) {
        const uint32_t idx = REV ? n - 1 - i : i;
        acc = OP::op(acc, a[idx]);
        a[idx] = acc;
    }
    float incl = acc;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float o = __shfl_up(incl, d, 64);
        if (lane >= (uint32_t)d) incl = OP::op(o, incl);
    }
    float excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = OP::id();
    for (uint32_t i = i0; i < i1; ++i) {
        const uint32_t idx = REV ? n - 1 - i : i;
        a[idx] = OP::op(excl, a[idx]);
    }
    __syncthreads();
}

// in-place inclusive sum of a[0..n) in LDS by one wave, as torch's CPU cumsum computes it: a float64 running sum, every output rounded to
// float32 (with float32 running sums the slopes of a narrow blur, thousands per unit, cost the cdf 1e-5).  REV: from the last element down.
template <bool REV>
__device__ __forceinline__ void nlr_rl_cumsum(float *a, uint32_t n, uint32_t lane) {
    const uint32_t per = (n + 63) / 64;
    const uint32_t i0 = min(n, lane * per), i1 = min(n, i0 + per);
    __syncthreads();
    double tot = 0.0;
    for (uint32_t i = i0; i < i1; ++i) tot += (double)a[REV ? n - 1 - i : i];
    double incl = tot;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(incl, d, 64);
        if (lane >= (uint32_t)d) incl += o;
    }
    double run = __shfl_up(incl, 1, 64);  // the lanes before this one
    if (lane == 0) run = 0.0;
    for (uint32_t i = i0; i < i1; ++i) {
        const uint32_t idx = REV ? n - 1 - i : i;
        run += (double)a[idx];
        a[idx] = (float)run;
    }
    __syncthreads();
}

// ---- distortion ---------------------------------------------------------------------------------------------------------------------
// t [S+1] and w [S] of the ray into LDS; X = D_k = sum_{j<k} w_j (u_k - u_j) as losses.distortion builds it: before = cumsum(w) - w,
// D = cumsum(before * du).  Ends with a barrier.
__device__ __forceinline__ void nlr_rl_dist_stage(const RayLossParams &A, uint32_t ray, float *T, float *W, float *X, uint32_t lane) {
    const uint32_t S = A.S;
    const float *t = A.sdist + (size_t)ray * (S + 1), *w = A.weights + (size_t)ray * S;
    __syncthreads();  // the previous ray's reads
    for (uint32_t k = lane; k <= S; k += 64) T[k] = t[k];
    for (uint32_t k = lane; k < S; k += 64) X[k] = W[k] = w[k];
    nlr_rl_cumsum<false>(X, S, lane);
    for (uint32_t k = lane; k < S; k += 64) {
        const float du = k == 0 ? 0.0f : 0.5f * (T[k + 1] + T[k]) - 0.5f * (T[k] + T[k - 1]);
        X[k] = (X[k] - W[k]) * du;
    }
    nlr_rl_cumsum<false>(X, S, lane);
}

// the ray's value 2 sum_k w_k D_k + sum_k w_k^2 (t_{k+1} - t_k) / 3, the same in every lane
__device__ __forceinline__ float nlr_rl_dist_ray(const RayLossParams &A, uint32_t ray, float *lds, uint32_t lane) {
    const uint32_t S = A.S;
    float *T = lds, *W = T + (S + 1), *X = W + S;
    nlr_rl_dist_stage(A, ray, T, W, X, lane);
    float a = 0.0f, b = 0.0f;
    for (uint32_t k = lane; k < S; k += 64) {
        const float w = W[k];
        a += w * X[k];
        b += w * w * (T[k + 1] - T[k]);
    }
    return 2.0f * nlr_wave_sum(a) + nlr_wave_sum(b) / 3.0f;
}

// d_weights of the ray: scale * (2 (D_k + E_k) + 2 w_k (t_{k+1} - t_k) / 3), E the mirror image of D
__device__ __forceinline__ void nlr_rl_dist_grad_ray(const RayLossParams &A, uint32_t ray, float scale, float *lds, uint32_t lane) {
    const uint32_t S = A.S;
    float *T = lds, *W = T + (S + 1), *X = W + S, *Y = X + S;
    nlr_rl_dist_stage(A, ray, T, W, X, lane);
    for (uint32_t k = lane; k < S; k += 64) Y[k] = W[k];
    nlr_rl_cumsum<true>(Y, S, lane);
    for (uint32_t k = lane; k < S; k += 64) {
        const float du = k + 1 == S ? 0.0f : 0.5f * (T[k + 2] + T[k + 1]) - 0.5f * (T[k + 1] + T[k]);
        Y[k] = (Y[k] - W[k]) * du;
    }
    nlr_rl_cumsum<true>(Y, S, lane);
    float *dw = A.dw + (size_t)ray * S;
    for (uint32_t k = lane; k < S; k += 64) dw[k] = scale * (2.0f * (X[k] + Y[k]) + 2.0f * W[k] * (T[k + 1] - T[k]) / 3.0f);
}

// ---- anti-aliased interlevel ----------------------------------------------------------------------------------------------------------
// element of the loss and its derivative with respect to wp: e = max(w_target - wp, 0) with a NaN kept, e^2 / (wp + 1e-5)
__device__ __forceinline__ float nlr_rl_excess(float wt, float wp) {
    const float d = wt - wp;
    return d < 0.0f ? 0.0f : d;
}

// level i of the ray: writes w_target, adds the kept elements to acc and their number to kept (per lane)
__device__ __forceinline__ void nlr_rl_anti_ray(const RayLossParams &A, uint32_t i, uint32_t ray, float *lds, uint32_t lane, float &acc,
                                                uint32_t &kept) {
    const uint32_t S = A.S, M = 2 * S + 2, Sp = A.pS[i];
    const float r = A.r[i], two_r = 2.0f * r;
    float *K = lds, *J = K + M, *V = J + M, *C = V + M, *F = C + M;  // C: the edges c, later the cdf
    const float *c = A.sdist + (size_t)ray * (S + 1), *w = A.weights + (size_t)ray * S;
    __syncthreads();  // the previous ray's reads
    for (uint32_t k = lane; k <= S; k += 64) C[k] = c[k];
    __syncthreads();
    // jump of the pdf at every edge, over 2r (pdf padded with 0 on both sides)
    for (uint32_t k = lane; k <= S; k += 64) {
        float pr = 0.0f, pl = 0.0f;
        if (k < S) {
            pr = w[k] / (C[k + 1] - C[k]);
            pr = pr > 10.0f ? 10.0f : pr;
        }
        if (k > 0) {
            pl = w[k - 1] / (C[k] - C[k - 1]);
            pl = pl > 10.0f ? 10.0f : pl;
        }
        V[k] = (pr - pl) / two_r;
    }
    __syncthreads();
    // merge: rank of c_k - r among the c + r (strictly below it) and of c_k + r among the c - r (at or below it)
    for (uint32_t k = lane; k <= S; k += 64) {
        const float a = C[k] - r, b = C[k] + r, j = V[k];
        uint32_t lo = 0, hi = S + 1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (C[mid] + r < a) lo = mid + 1; else hi = mid;
        }
        const uint32_t pa = k + lo;
        lo = 0, hi = S + 1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (C[mid] - r <= b) lo = mid + 1; else hi = mid;
        }
        const uint32_t pb = k + lo;
        K[pa] = a;
        J[pa] = j;
        K[pb] = b;
        J[pb] = -j;
    }
    nlr_rl_cumsum<false>(J, M, lane);  // slope after every knot (the last one is not used)
    for (uint32_t m = lane; m < M; m += 64) V[m] = m == 0 ? 0.0f : (K[m] - K[m - 1]) * J[m - 1];
    nlr_rl_cumsum<false>(V, M, lane);
    for (uint32_t m = lane; m < M; m += 64) {
        const float v = V[m];
        V[m] = v < 0.0f ? 0.0f : v;  // clamp_min(0) of the finished scan; a NaN stays
    }
    __syncthreads();
    for (uint32_t m = lane; m < M; m += 64) {
        C[m] = m == 0 ? 0.0f : 0.5f * (V[m] + V[m - 1]) * (K[m] - K[m - 1]);
        J[m] = V[m];
    }
    nlr_rl_cumsum<false>(C, M, lane);  // cdf
    nlr_rl_scan<RlMin, true>(J, M, lane);   // min of val over the knots from here on
    nlr_rl_scan<RlMax, false>(V, M, lane);  // max of val over the knots up to here
    // the cdf at the proposal edges
    const float *cp = A.psd[i] + (size_t)ray * (Sp + 1);
    for (uint32_t j = lane; j <= Sp; j += 64) {
        const float q = cp[j];
        uint32_t lo = 0, hi = M;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (K[mid] <= q) lo = mid + 1; else hi = mid;
        }
        const uint32_t cnt = lo, l = cnt > 0 ? cnt - 1 : 0, h = min(cnt, M - 1);
        const float x0 = K[l], x1 = K[h], p0 = V[l], p1 = J[h];
        const float frac = nlr_nan0_clip01((q - x0) / (x1 - x0));
        F[j] = C[l] + (q - x0) * (p0 + p1 * frac + p0 * (1.0f - frac)) / 2.0f;
    }
    __syncthreads();
    const float *wp = A.pw[i] + (size_t)ray * Sp;
    const uint8_t *mask = A.pm[i] ? A.pm[i] + (size_t)ray * Sp : nullptr;
    float *wt = A.wt[i] + (size_t)ray * Sp;
    for (uint32_t j = lane; j < Sp; j += 64) {
        const float t = F[j + 1] - F[j], p = wp[j], e = nlr_rl_excess(t, p);
        wt[j] = t;
        if (!mask || !mask[j]) {
            acc += e * e / (p + 1e-5f);
            ++kept;
        }
    }
}

__global__ void __launch_bounds__(64) nlr_ray_losses_fwd_kernel(RayLossParams A, float *__restrict__ part, uint32_t *__restrict__ cnt) {
    extern __shared__ __align__(16) float lds[];
    const uint32_t lane = threadIdx.x, term = blockIdx.y;
    const uint32_t ray0 = blockIdx.x * NLR_RL_RPB, ray1 = min(A.N, ray0 + NLR_RL_RPB);
    float acc = 0.0f;
    uint32_t kept = 0;
    if (term == 0) {
        for (uint32_t ray = ray0; ray < ray1; ++ray) acc += nlr_rl_dist_ray(A, ray, lds, lane);
        kept = ray1 - ray0;
    } else {
        for (uint32_t ray = ray0; ray < ray1; ++ray) nlr_rl_anti_ray(A, term - 1, ray, lds, lane, acc, kept);
        acc = nlr_wave_sum(acc);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) kept += __shfl_xor(kept, d, 64);
    }
    if (lane == 0) {
        part[(size_t)term * gridDim.x + blockIdx.x] = acc;
        cnt[(size_t)term * gridDim.x + blockIdx.x] = kept;
    }
}

// one wave per term: stats[term] = the sum, stats[T + term] = the count (N rays / kept samples), terms[term] = sum / count (0 / 0 = NaN:
// the reference's mean of nothing)
__global__ void __launch_bounds__(64) nlr_ray_losses_sum_kernel(const float *__restrict__ part, const uint32_t *__restrict__ cnt, uint32_t blocks,
                                                                float *__restrict__ terms, float *__restrict__ stats) {
    const uint32_t term = blockIdx.x, T = gridDim.x;
    double a = 0.0;
    unsigned long long n = 0;
    for (uint32_t b = threadIdx.x; b < blocks; b += 64) {
        a += (double)part[(size_t)term * blocks + b];
        n += cnt[(size_t)term * blocks + b];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a += __shfl_xor(a, d, 64);
        n += __shfl_xor(n, d, 64);
    }
    if (threadIdx.x == 0) {
        stats[term] = (float)a;
        stats[T + term] = (float)n;
        terms[term] = (float)(a / (double)n);
    }
}

__global__ void __launch_bounds__(64) nlr_ray_losses_bwd_kernel(RayLossParams A, const float *__restrict__ stats,
                                                                const float *__restrict__ g_terms) {
    extern __shared__ __align__(16) float lds[];
    const uint32_t lane = threadIdx.x, term = blockIdx.y, T = 1 + A.n_prop;
    const uint32_t ray0 = blockIdx.x * NLR_RL_RPB, ray1 = min(A.N, ray0 + NLR_RL_RPB);
    const float scale = g_terms[term] / stats[T + term];
    if (term == 0) {
        for (uint32_t ray = ray0; ray < ray1; ++ray) nlr_rl_dist_grad_ray(A, ray, scale, lds, lane);
        return;
    }
    // elementwise on the kept samples: d/dwp of e^2 / (wp + 1e-5); a level without kept samples has scale = g / 0 and nothing to apply it to
    const uint32_t i = term - 1, Sp = A.pS[i];
    const size_t e0 = (size_t)ray0 * Sp, e1 = (size_t)ray1 * Sp;
    const float *wt = A.wt[i], *wp = A.pw[i];
    const uint8_t *mask = A.pm[i];
    float *d = A.dpw[i];
    for (size_t x = e0 + lane; x < e1; x += 64) {
        float g = 0.0f;
        if (!mask || !mask[x]) {
            const float p = wp[x], e = nlr_rl_excess(wt[x], p), den = p + 1e-5f;
            g = scale * (-2.0f * e / den - e * e / (den * den));
        }
        d[x] = g;
    }
}

// LDS floats of a launch: the distortion rays need t [S + 1] and `dist_arrays` arrays of S (forward: w, D; backward: w, D, E), the anti
// rays 4 arrays of 2S + 2 and the cdf at the largest level's edges
static inline size_t nlr_rl_lds_floats(uint32_t S, const uint32_t *pS, uint32_t n_prop, uint32_t dist_arrays) {
    size_t n = (size_t)S + 1 + (size_t)dist_arrays * S;
    for (uint32_t i = 0; i < n_prop; ++i) {
        const size_t anti = 4 * ((size_t)2 * S + 2) + pS[i] + 1;
        n = anti > n ? anti : n;
    }
    return (n + 3) & ~(size_t)3;
}

static int nlr_rl_check(const char *fn, const float *sdist, const float *weights, uint32_t N, uint32_t S, const float *const *prop_sdist,
                        const float *const *prop_weights, const uint32_t *prop_S_host, const float *pulse_width_host, uint32_t n_prop,
                        const void *workspace, size_t workspace_bytes) {
    NLR_CHECK_ARG(sdist, "%s: sdist is NULL", fn);
    NLR_CHECK_ARG(weights, "%s: weights is NULL", fn);
    NLR_CHECK_ARG(N >= 1, "%s: N = 0 rays", fn);
    NLR_CHECK_ARG(S >= 1 && S <= NLR_RAY_LOSSES_MAX_S, "%s: S = %u outside [1, %d]", fn, S, NLR_RAY_LOSSES_MAX_S);
    NLR_CHECK_ARG(n_prop <= NLR_RAY_LOSSES_MAX_PROP, "%s: n_prop = %u outside [0, %d]", fn, n_prop, NLR_RAY_LOSSES_MAX_PROP);
    if (n_prop) {
        NLR_CHECK_ARG(prop_sdist, "%s: prop_sdist is NULL with n_prop = %u", fn, n_prop);
        NLR_CHECK_ARG(prop_weights, "%s: prop_weights is NULL with n_prop = %u", fn, n_prop);
        NLR_CHECK_ARG(prop_S_host, "%s: prop_S_host is NULL with n_prop = %u", fn, n_prop);
        NLR_CHECK_ARG(pulse_width_host, "%s: pulse_width_host is NULL with n_prop = %u", fn, n_prop);
    }
    for (uint32_t i = 0; i < n_prop; ++i) {
        NLR_CHECK_ARG(prop_sdist[i], "%s: prop_sdist[%u] is NULL", fn, i);
        NLR_CHECK_ARG(prop_weights[i], "%s: prop_weights[%u] is NULL", fn, i);
        NLR_CHECK_ARG(prop_S_host[i] >= 1 && prop_S_host[i] <= NLR_RAY_LOSSES_MAX_S, "%s: prop_S_host[%u] = %u outside [1, %d]", fn, i,
                      prop_S_host[i], NLR_RAY_LOSSES_MAX_S);
        NLR_CHECK_ARG(isfinite(pulse_width_host[i]) && pulse_width_host[i] > 0.0f, "%s: pulse_width_host[%u] = %g is not finite and > 0", fn, i,
                      (double)pulse_width_host[i]);
    }
    NLR_CHECK_ARG(workspace, "%s: workspace is NULL", fn);
    NLR_CHECK_ARG(workspace_bytes >= nlr_rl_ws_bytes(N, n_prop), "%s: workspace_bytes = %zu, nlr_ray_losses_workspace_bytes(%u, %u) = %zu", fn,
                  workspace_bytes, N, n_prop, nlr_rl_ws_bytes(N, n_prop));
    return NLR_OK;
}

static RayLossParams nlr_rl_params(const float *sdist, const float *weights, uint32_t N, uint32_t S, const float *const *prop_sdist,
                                   const float *const *prop_weights, const uint8_t *const *prop_obj_mask, const uint32_t *prop_S_host,
                                   const float *pulse_width_host, uint32_t n_prop) {
    RayLossParams A;
    memset(&A, 0, sizeof(A));
    A.sdist = sdist, A.weights = weights, A.N = N, A.S = S, A.n_prop = n_prop;
    for (uint32_t i = 0; i < n_prop; ++i) {
        A.psd[i] = prop_sdist[i], A.pw[i] = prop_weights[i], A.pm[i] = prop_obj_mask ? prop_obj_mask[i] : nullptr;
        A.pS[i] = prop_S_host[i], A.r[i] = pulse_width_host[i];
    }
    return A;
}

extern "C" int nlr_ray_losses_forward(const float *sdist, const float *weights, uint32_t N, uint32_t S, const float *const *prop_sdist,
                                      const float *const *prop_weights, const uint8_t *const *prop_obj_mask, const uint32_t *prop_S_host,
                                      const float *pulse_width_host, uint32_t n_prop, float *terms, float *stats, float *const *w_target,
                                      void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "ray_losses_forward";
    if (int rc = nlr_rl_check(fn, sdist, weights, N, S, prop_sdist, prop_weights, prop_S_host, pulse_width_host, n_prop, workspace, workspace_bytes))
        return rc;
    NLR_CHECK_ARG(terms, "%s: terms is NULL", fn);
    NLR_CHECK_ARG(stats, "%s: stats is NULL", fn);
    NLR_CHECK_ARG(!n_prop || w_target, "%s: w_target is NULL with n_prop = %u", fn, n_prop);
    for (uint32_t i = 0; i < n_prop; ++i) NLR_CHECK_ARG(w_target[i], "%s: w_target[%u] is NULL", fn, i);
    RayLossParams A = nlr_rl_params(sdist, weights, N, S, prop_sdist, prop_weights, prop_obj_mask, prop_S_host, pulse_width_host, n_prop);
    for (uint32_t i = 0; i < n_prop; ++i) A.wt[i] = w_target[i];
    hipStream_t st = (hipStream_t)stream;
    const uint32_t blocks = nlr_rl_blocks(N), T = 1 + n_prop;
    float *part = (float *)workspace;
    uint32_t *cnt = (uint32_t *)(part + (size_t)T * blocks);
    hipLaunchKernelGGL(nlr_ray_losses_fwd_kernel, dim3(blocks, T), dim3(64), nlr_rl_lds_floats(S, A.pS, n_prop, 2) * sizeof(float), st, A, part, cnt);
    NLR_LAUNCH_CHECK("nlr_ray_losses_fwd_kernel");
    hipLaunchKernelGGL(nlr_ray_losses_sum_kernel, dim3(T), dim3(64), 0, st, part, cnt, blocks, terms, stats);
    NLR_LAUNCH_CHECK("nlr_ray_losses_sum_kernel");
    return NLR_OK;
}

extern "C" int nlr_ray_losses_backward(const float *sdist, const float *weights, uint32_t N, uint32_t S, const float *const *prop_sdist,
                                       const float *const *prop_weights, const uint8_t *const *prop_obj_mask, const uint32_t *prop_S_host,
                                       const float *pulse_width_host, uint32_t n_prop, const float *stats, const float *g_terms,
                                       const float *const *w_target, float *d_weights, float *const *d_prop_weights, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    const char *fn = "ray_losses_backward";
    if (int rc = nlr_rl_check(fn, sdist, weights, N, S, prop_sdist, prop_weights, prop_S_host, pulse_width_host, n_prop, workspace, workspace_bytes))
        return rc;
    NLR_CHECK_ARG(stats, "%s: stats is NULL", fn);
    NLR_CHECK_ARG(g_terms, "%s: g_terms is NULL", fn);
    NLR_CHECK_ARG(d_weights, "%s: d_weights is NULL", fn);
    NLR_CHECK_ARG(!n_prop || w_target, "%s: w_target is NULL with n_prop = %u", fn, n_prop);
    NLR_CHECK_ARG(!n_prop || d_prop_weights, "%s: d_prop_weights is NULL with n_prop = %u", fn, n_prop);
    for (uint32_t i = 0; i < n_prop; ++i) {
        NLR_CHECK_ARG(w_target[i], "%s: w_target[%u] is NULL", fn, i);
        NLR_CHECK_ARG(d_prop_weights[i], "%s: d_prop_weights[%u] is NULL", fn, i);
    }
    RayLossParams A = nlr_rl_params(sdist, weights, N, S, prop_sdist, prop_weights, prop_obj_mask, prop_S_host, pulse_width_host, n_prop);
    for (uint32_t i = 0; i < n_prop; ++i) A.wt[i] = const_cast<float *>(w_target[i]), A.dpw[i] = d_prop_weights[i];
    A.dw = d_weights;
    hipLaunchKernelGGL(nlr_ray_losses_bwd_kernel, dim3(nlr_rl_blocks(N), 1 + n_prop), dim3(64), nlr_rl_lds_floats(S, nullptr, 0, 3) * sizeof(float),
                       (hipStream_t)stream, A, stats, g_terms);
    NLR_LAUNCH_CHECK("nlr_ray_losses_bwd_kernel");
    return NLR_OK;
}
