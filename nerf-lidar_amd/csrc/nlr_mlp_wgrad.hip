// Weight and bias gradients of the fused training NerfMLP (header section 6b) as one MFMA kernel plus a slab reduce.
//
//   dW[o, i] = sum_m gacts[m, o] . x[m, i]      db[o] = sum_m gacts[m, o]
//
// for every Linear of the plan, x being a column block of `acts`, the grid features or the per-ray direction encoding (table in the
// header).  Both operands are row-major with the REDUCTION index (the sample m) as the row, so neither is in MFMA operand order.
// Rows are staged into LDS as they lie in memory (16-byte global loads; f32 sources are rounded to bf16 on the way) and both
// operands of v_mfma_f32_16x16x32_bf16 are read from that image with ds_read_b64_tr_b16, the transposed LDS read of gfx950.
//
// Work split.  A job is one 128 x 128 block of one dW: 128 columns of gacts x 128 columns of an input block.  The grid is
// jobs x NLR_WG_SLICES workgroups; workgroup b does job b / slices on M slice b % slices, so that with the round-robin placement of
// workgroups on the 8 XCDs all jobs of one slice run on one XCD and the re-reads of a row range (the bottleneck block feeds four
// Linears) meet in that XCD's L2.  All workgroups are resident at once (at most 64 jobs x 8 slices on 256 CUs x 2), walk their slice
// front to back and keep their block of dW in registers the whole way: a workgroup writes its result ONCE, into its slice's f32 slab
// of the workspace, in the layout of d_params.  nlr_mlp_wgrad_reduce_kernel then sums the slabs in slice order.  No atomics anywhere:
// the order of every sum is fixed by (M, S, plan), so two calls on the same inputs give the same bits.
//
// Inside a workgroup: 4 waves = 2 (o halves) x 2 (i halves), each 4 x 4 tiles of 16 x 16 (64 accumulator registers).  A chunk of
// 64 rows is two k-steps.  LDS row r of a k-step holds sample r of it; the 16-lane group g of a wave reads rows 4g .. 4g+3 and
// 16 + 4g .. 16 + 4g+3 as its 8 k values.  That is a permutation of the k order of the MFMA's operand map, the same one for A and
// for B, which a sum over k does not see; it puts the 8 rows that one 32-lane half reads side by side, and with a row pitch of
// 288 B = 8 banks (mod 64) those 8 rows x 32 B cover the 64 banks once: no bank conflict by the bank rule of the transposed read.
// Rows past M and columns past a block's width are staged as zeros (every lane of a transposed read supplies an address, EXEC is
// full: the branches around the MFMA section are wave-uniform).
#include <type_traits>

#include "nlr_kernels.h"
#include "nlr_train_plan.h"

#define NLR_WG_SLICES 8      // M slices = f32 slabs in the workspace
#define NLR_WG_MAX_JOBS 64   // largest plan (W = 256, D = 10, both heads): 59
#define NLR_WG_CH 64         // rows per staged chunk
#define NLR_WG_PITCH 288     // bytes per LDS row: 128 bf16 + 32 B

struct WgJob {
    uint16_t g_col;           // first column of gacts of this block (a multiple of 8)
    uint16_t o_lo, o_hi;      // tile rows [o_lo, o_hi) are rows 0 .. of the destination
    uint16_t x_src, x_col;    // 0 acts, 1 features, 2 enc; first column
    uint16_t n_in;            // valid columns of the input block (<= 128)
    uint16_t dst_ld;          // `in` of the Linear
    uint16_t has_bias;
    uint16_t color;           // 1: a view layer or rgb_layer, reduced over the rows with colour supervision [0, M_color) only
    uint32_t dst, bias;       // offsets into d_params of dW[first row][first column] and of db[first row]
};

struct WgParams {
    uint32_t M, M_color, S, F, E, ld_a, ld_g, n_slices, n_params;
    const float *feat, *enc;
    const __bf16 *acts, *gacts;
    float *slab;
    WgJob jobs[NLR_WG_MAX_JOBS];
};

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // 16 bytes as one register quad (HIP's uint4 is a struct)
typedef __attribute__((address_space(3))) bf16x4 *nlr_l4ptr;

__device__ __forceinline__ bf16x8 nlr_tr_frag(const unsigned char *p) {
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((nlr_l4ptr)p);
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((nlr_l4ptr)(p + 16 * NLR_WG_PITCH));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

__device__ __forceinline__ u32x4 nlr_pack8(const f32x4 &a, const f32x4 &b) {
    bf16x8 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (__bf16)a[i], v[4 + i] = (__bf16)b[i];  // round to nearest even
    return __builtin_bit_cast(u32x4, v);
}

__global__ void __launch_bounds__(256, 2) nlr_mlp_wgrad_kernel(WgParams P) {
    __shared__ __align__(16) unsigned char lds[2 * NLR_WG_CH * NLR_WG_PITCH];
    unsigned char *const lds_g = lds, *const lds_x = lds + NLR_WG_CH * NLR_WG_PITCH;
    const uint32_t slice = blockIdx.x % P.n_slices, jid = blockIdx.x / P.n_slices;
    const WgJob J = P.jobs[jid];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // uniform
    const uint32_t x_src = J.x_src;
    const uint32_t oh = wave >> 1, ih = wave & 1;
    // this job's rows [0, Mj) in chunks, dealt to the n_slices slabs front to back; a slice (or a whole job: M_color = 0) without
    // rows runs no chunk and writes its zero accumulators, so the reduce reads defined memory everywhere
    const uint32_t Mj = J.color ? P.M_color : P.M;
    const uint32_t n_chunks = (Mj + NLR_WG_CH - 1) / NLR_WG_CH, chunks_per_slice = (n_chunks + P.n_slices - 1) / P.n_slices;
    const uint32_t c_begin = min(slice * chunks_per_slice, n_chunks);
    const uint32_t c_end = min(c_begin + chunks_per_slice, n_chunks);
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    const u32x4 zero16 = {0u, 0u, 0u, 0u};

    // staging: item id = tid + 256 k is 16-byte unit (id & 15) of row (id >> 4): 16 consecutive lanes read one 256-byte line
    const uint32_t unit = tid & 15, row0 = tid >> 4;
    const bool g_on = 8 * unit < J.o_hi, x_on = 8 * unit < J.n_in;
    u32x4 rg[4], rx[4];
    auto fetch = [&](uint32_t c) {
        const uint32_t m0 = c * NLR_WG_CH + row0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t m = m0 + 16 * k;
            rg[k] = (m < Mj && g_on) ? *reinterpret_cast<const u32x4 *>(P.gacts + (size_t)m * P.ld_g + J.g_col + 8 * unit) : zero16;
        }
        if (x_src == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t m = m0 + 16 * k;
                rx[k] = (m < Mj && x_on) ? *reinterpret_cast<const u32x4 *>(P.acts + (size_t)m * P.ld_a + J.x_col + 8 * unit) : zero16;
            }
        } else if (x_src == 1) {  // grid features, f32: 8 unit < n_in = F and F % 4 == 0
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t m = m0 + 16 * k;
                const float *f = P.feat + (size_t)m * P.F + 8 * unit;
                const f32x4 a = (m < Mj && x_on) ? *reinterpret_cast<const f32x4 *>(f) : zero4;
                const f32x4 b = (m < Mj && 8 * unit + 4 < J.n_in) ? *reinterpret_cast<const f32x4 *>(f + 4) : zero4;
                rx[k] = nlr_pack8(a, b);
            }
        } else {  // direction encoding of the sample's ray, f32 [M / S, 32]: 8 unit < E <= 32
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t m = m0 + 16 * k;
                const float *e = P.enc + (size_t)(m / P.S) * 32 + 8 * unit;
                f32x4 a = zero4, b = zero4;
                if (m < Mj && x_on) a = *reinterpret_cast<const f32x4 *>(e), b = *reinterpret_cast<const f32x4 *>(e + 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    a[i] = 8 * unit + i < P.E ? a[i] : 0.0f;
                    b[i] = 8 * unit + 4 + i < P.E ? b[i] : 0.0f;
                }
                rx[k] = nlr_pack8(a, b);
            }
        }
    };

    // this wave's share: tile rows 64 oh + 16 ot, tile columns 64 ih + 16 it
    const bool active = 64 * oh < J.o_hi && 64 * ih < J.n_in;
    const uint32_t n_ot = active ? min(4u, (J.o_hi - 64 * oh + 15) / 16) : 0;
    const bool do_bias = active && ih == 0 && J.has_bias;
    f32x4 acc[4][4], bacc[4];
#pragma unroll
    for (int ot = 0; ot < 4; ++ot) {
        bacc[ot] = zero4;
#pragma unroll
        for (int it = 0; it < 4; ++it) acc[ot][it] = zero4;
    }
    bf16x8 ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (__bf16)1.0f;
    // transposed read: lane 4 q + p of group g supplies row 4 g + q (and 16 + that), columns 4 p .. 4 p + 3 of the tile
    const uint32_t tr_off = (4 * (lane >> 4) + ((lane >> 2) & 3)) * NLR_WG_PITCH + (lane & 3) * 8;
    const unsigned char *const ga = lds_g + tr_off + oh * 128, *const xa = lds_x + tr_off + ih * 128;

    auto mma = [&](auto full, auto bias) {
        constexpr bool FULL = decltype(full)::value, BIAS = decltype(bias)::value;
#pragma unroll
        for (int ks = 0; ks < NLR_WG_CH / 32; ++ks) {
            bf16x8 xb[4];
#pragma unroll
            for (int it = 0; it < 4; ++it) xb[it] = nlr_tr_frag(xa + ks * 32 * NLR_WG_PITCH + it * 32);
#pragma unroll
            for (int ot = 0; ot < 4; ++ot) {
                if (FULL || ot < (int)n_ot) {
                    const bf16x8 gf = nlr_tr_frag(ga + ks * 32 * NLR_WG_PITCH + ot * 32);
#pragma unroll
                    for (int it = 0; it < 4; ++it) acc[ot][it] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf, xb[it], acc[ot][it], 0, 0, 0);
                    if (BIAS || (!FULL && do_bias)) bacc[ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf, ones, bacc[ot], 0, 0, 0);
                }
            }
        }
    };

    if (c_begin < c_end) fetch(c_begin);
    for (uint32_t c = c_begin; c < c_end; ++c) {
        __syncthreads();  // the previous chunk's reads are done
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t o = (row0 + 16 * k) * NLR_WG_PITCH + unit * 16;
            *reinterpret_cast<u32x4 *>(lds_g + o) = rg[k];
            *reinterpret_cast<u32x4 *>(lds_x + o) = rx[k];
        }
        __syncthreads();
        if (c + 1 < c_end) fetch(c + 1);  // in flight during the MFMAs
        // whole-tile waves run a branch-free body (with or without the bias MFMA); partial ones test every tile row, wave-uniformly
        if (n_ot == 4 && !do_bias) mma(std::true_type(), std::false_type());
        else if (n_ot == 4) mma(std::true_type(), std::true_type());
        else if (active) mma(std::false_type(), std::false_type());
    }

    // result tile: column = lane & 15 (i), row = 4 (lane >> 4) + register (o); padded rows and columns are not written
    float *const slab = P.slab + (size_t)slice * P.n_params;
    if (active) {
#pragma unroll
        for (int ot = 0; ot < 4; ++ot) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t o = 64 * oh + 16 * ot + 4 * (lane >> 4) + r;
                if (o >= J.o_lo && o < J.o_hi) {
#pragma unroll
                    for (int it = 0; it < 4; ++it) {
                        const uint32_t i = 64 * ih + 16 * it + (lane & 15);
                        if (i < J.n_in) slab[J.dst + (size_t)(o - J.o_lo) * J.dst_ld + i] = acc[ot][it][r];
                    }
                    if (do_bias && (lane & 15) == 0) slab[J.bias + (o - J.o_lo)] = bacc[ot][r];
                }
            }
        }
    }
}

// d_params[i] = slab_0[i] + slab_1[i] + ..: one fixed order
__global__ void __launch_bounds__(256) nlr_mlp_wgrad_reduce_kernel(const float *__restrict__ slab, uint32_t n_slices, uint32_t n,
                                                                  float *__restrict__ out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = slab[i];
    for (uint32_t k = 1; k < n_slices; ++k) s += slab[(size_t)k * n + i];
    out[i] = s;
}

// ---- the job list of a plan: every (Linear, 128 output rows, 128 input columns) of the plan's layer table ---------------------------
static int build_jobs(const NlrTrainPlan *p, WgJob *jobs, uint32_t *n_jobs) {
    uint32_t n = 0;
    *n_jobs = 0;
    for (const TrainLinear &l : p->linears) {
        uint32_t n_in_total = 0;
        for (uint32_t k = 0; k < l.n_in; ++k) n_in_total += l.in[k].n;
        for (uint32_t o0 = 0; o0 < l.n_out; o0 += 128) {
            uint32_t i0 = 0;
            bool first = true;
            for (uint32_t k = 0; k < l.n_in; ++k) {
                for (uint32_t c = 0; c < l.in[k].n; c += 128) {
                    if (n >= NLR_WG_MAX_JOBS) return NLR_ERR_UNSUPPORTED;
                    WgJob &j = jobs[n++];
                    const uint32_t rows = l.n_out - o0 < 128 ? l.n_out - o0 : 128, cols = l.in[k].n - c < 128 ? l.in[k].n - c : 128;
                    j.g_col = (uint16_t)(l.g_col - l.o_off + o0);
                    j.o_lo = (uint16_t)l.o_off, j.o_hi = (uint16_t)(l.o_off + rows);
                    j.x_src = (uint16_t)l.in[k].src, j.x_col = (uint16_t)(l.in[k].col + c), j.n_in = (uint16_t)cols;
                    j.dst_ld = (uint16_t)n_in_total;
                    j.has_bias = first ? 1 : 0;
                    j.color = (uint16_t)l.color;
                    j.dst = l.w_off + o0 * n_in_total + i0 + c;
                    j.bias = l.b_off + o0;
                    first = false;
                }
                i0 += l.in[k].n;
            }
        }
    }
    *n_jobs = n;
    return NLR_OK;
}

// NLR_WG_SLICES f32 slabs of n_params floats: independent of M
extern "C" size_t nlr_mlp_train_wgrad_workspace_bytes(const NlrTrainPlan *p, uint32_t M) {
    (void)M;
    return p ? (size_t)NLR_WG_SLICES * p->n_params * sizeof(float) : 0;
}

static int train_wgrad(const NlrTrainPlan *p, uint32_t M, uint32_t M_color, uint32_t S, const float *features, const float *enc,
                       const void *acts, const void *gacts, float *d_params, void *workspace, void *stream) {
    WgParams P;
    memset(&P, 0, sizeof(P));
    uint32_t n_jobs = 0;
    const int rc = build_jobs(p, P.jobs, &n_jobs);
    if (rc != NLR_OK || n_jobs == 0) NLR_FAIL(rc ? rc : NLR_ERR_UNSUPPORTED, "mlp_train_wgrad: no job list for this plan");
    P.M = M, P.M_color = M_color, P.S = S, P.F = p->F, P.E = p->E, P.ld_a = p->act_w, P.ld_g = p->act_w + 64, P.n_params = p->n_params;
    const uint32_t n_chunks = (M + NLR_WG_CH - 1) / NLR_WG_CH;
    P.n_slices = n_chunks < NLR_WG_SLICES ? n_chunks : NLR_WG_SLICES;  // by M: the slab layout is the same for every job
    P.feat = features, P.enc = enc, P.acts = (const __bf16 *)acts, P.gacts = (const __bf16 *)gacts;
    P.slab = (float *)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nlr_mlp_wgrad_kernel, dim3(n_jobs * P.n_slices), dim3(256), 0, st, P);
    NLR_LAUNCH_CHECK("nlr_mlp_wgrad_kernel");
    hipLaunchKernelGGL(nlr_mlp_wgrad_reduce_kernel, dim3((p->n_params + 255) / 256), dim3(256), 0, st, (const float *)workspace, P.n_slices,
                       p->n_params, d_params);
    NLR_LAUNCH_CHECK("nlr_mlp_wgrad_reduce_kernel");
    return NLR_OK;
}

#define NLR_WGRAD_ARGS(what)                                                                                                               \
    NLR_CHECK_ARG(p, what ": plan is NULL");                                                                                               \
    NLR_CHECK_ARG(features, what ": features is NULL");                                                                                    \
    NLR_CHECK_ARG(enc, what ": enc is NULL");                                                                                              \
    NLR_CHECK_ARG(acts, what ": acts is NULL");                                                                                            \
    NLR_CHECK_ARG(gacts, what ": gacts is NULL");                                                                                          \
    NLR_CHECK_ARG(d_params, what ": d_params is NULL");                                                                                    \
    NLR_CHECK_ARG(workspace, what ": workspace is NULL");                                                                                  \
    NLR_CHECK_ARG(M > 0, what ": M is 0");                                                                                                 \
    NLR_CHECK_ARG(S > 0 && M % S == 0, what ": M = %u is not a multiple of S = %u (M %% S != 0)", M, S)
#define NLR_WGRAD_WORKSPACE(what)                                                                                                          \
    const size_t need = nlr_mlp_train_wgrad_workspace_bytes(p, M);                                                                         \
    if (workspace_bytes < need)                                                                                                            \
        NLR_FAIL(NLR_ERR_WORKSPACE, what ": workspace_bytes %zu B < nlr_mlp_train_wgrad_workspace_bytes() = %zu B", workspace_bytes, need)

extern "C" int nlr_mlp_train_wgrad(const NlrTrainPlan *p, uint32_t M, uint32_t S, const float *features, const float *enc, const void *acts,
                                   const void *gacts, float *d_params, void *workspace, size_t workspace_bytes, void *stream) {
    NLR_WGRAD_ARGS("mlp_train_wgrad");
    NLR_WGRAD_WORKSPACE("mlp_train_wgrad");
    return train_wgrad(p, M, M, S, features, enc, acts, gacts, d_params, workspace, stream);
}

// view-layer and rgb_layer jobs reduce over rows [0, M_color) and never read a later row of acts / gacts; the others over all M
extern "C" int nlr_mlp_train_wgrad_split(const NlrTrainPlan *p, uint32_t M, uint32_t M_color, uint32_t S, const float *features,
                                         const float *enc, const void *acts, const void *gacts, float *d_params, void *workspace,
                                         size_t workspace_bytes, void *stream) {
    NLR_WGRAD_ARGS("mlp_train_wgrad_split");
    NLR_CHECK_ARG(M_color <= M, "mlp_train_wgrad_split: M_color = %u exceeds M = %u (M_color > M)", M_color, M);
    NLR_CHECK_ARG(M_color % S == 0, "mlp_train_wgrad_split: M_color = %u is not a multiple of S = %u (M_color %% S != 0)", M_color, S);
    NLR_WGRAD_WORKSPACE("mlp_train_wgrad_split");
    return train_wgrad(p, M, M_color, S, features, enc, acts, gacts, d_params, workspace, stream);
}
