// Fused NerfMLP forward-with-saved-activations and backward for training (scope row f-3).
//
// Replaces, between the hash-grid features and the per-sample heads, what autograd does for the reference's Linear stack in
// `loss.backward()` (Z/train.py:272-281,459 through ZI/models.py:1116-1251): density_layer, sem_layer, intensity_layer,
// lin_second_stage_0..D-1 (+ skip concat), rgb_layer, their ReLUs, softplus / softmax / sigmoid.
//
// Same machinery as the inference kernel (nlr_mlp_kernel.h): transposed chain on v_mfma_f32_16x16x32_bf16, activations and
// activation GRADIENTS in registers as B operands, weights as 1 KiB A fragments streamed from a tape through the LDS ring.
//   forward  tape: D0 D2 [H1 H2] V0 V1 L2..L(D-1) RGB, plain bf16 (mixed-precision training), one wave = 32 samples (2 column
//            tiles), every layer's output also stored row-major in `acts` [M, act_w] bf16 (inputs of the weight gradients and the
//            ReLU masks of the backward)
//   backward tape: RGB^T L(D-1)^T..L2^T V1a^T H2^T BIG D2^T D0^T with BIG = [V1 skip^T | V0^T | H1^T | e_0]: the gradient of the
//            bottleneck collects its four sources (skip concat, view layer 0, heads, raw density) in ONE accumulator chain.
//            Every layer's pre-activation gradient is stored row-major in `gacts`; the gradient of the features goes out in f32.
// Weight gradients are GEMMs over the saved tensors (dW_l = gacts_l^T . acts_{l-1}, M-long reductions), as are the bias sums:
// nlr_mlp_train_wgrad (nlr_mlp_wgrad.hip) computes all of them in one MFMA kernel plus a slab reduce; nerflidar_hip/training.py
// also keeps the older form, library GEMMs on the host side, as its default.
// The plan (nlr_train_plan.h) holds ONE table of the Linear layers: flat-parameter offsets, the columns of acts / gacts each reads and
// writes, which ones see the colour rows only.  plan_build derives from it the index maps of both tapes (with and without the view MLP)
// and of the bias block, without touching a device; nlr_mlp_wgrad.hip derives its job list from it, the host side its GEMMs
// (nlr_train_linear_table).  The tapes are re-packed on the device from the flat parameter buffer before every step (nlr_train_pack:
// one gather through those index maps).
#include <vector>

#include "nlr_mlp_kernel.h"
#include "nlr_train_plan.h"

struct TrainParams {
    uint32_t M, S, F, depth, K, int_row, act_w;  // M: one past the last row of this launch
    uint32_t row0, ldm;                          // first row of this launch; samples of the channel-major tensors (rgb [3, ldm], ..)
    const float *feat;   // [M, F] f32
    const float *enc;    // [N, 32]
    const uint4 *tape;
    uint32_t tape_chunks;
    const float *bias_all;
    uint32_t bias_count;
    float density_bias, rgb_premul, rgb_bias, rgb_padding;
    float *density, *rgb, *sem, *inten;  // forward outputs (backward: inputs): [M], [3,M], [K,M], [M]
    __bf16 *acts;                        // [M, act_w]
    const float *g_density, *g_rgb, *g_sem, *g_inten;  // upstream gradients, same layouts; any may be null
    __bf16 *gacts;                       // [M, act_w + 64]
    float *d_feat;                       // [M, F]
};

// row-major [M, ld] bf16 <-> B-operand tiles: lane (col, q) of column tile n holds features c0 + 4q .. +3 (elements 0..3) and
// c0 + 16 + 4q .. +3 (elements 4..7) of sample s0 + 16n + col: two 8-byte accesses per tile
__device__ __forceinline__ void nlr_store_bt(__bf16 *base, uint32_t ld, uint32_t s0, uint32_t M, int col, int q, uint32_t c0, const BT<2> &t) {
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const uint32_t smp = s0 + 16 * n + col;
        if (smp < M) {
            const uint4 v = __builtin_bit_cast(uint4, t.n[n]);
            __bf16 *p = base + (size_t)smp * ld + c0 + 4 * q;
            *reinterpret_cast<uint2 *>(p) = make_uint2(v.x, v.y);
            *reinterpret_cast<uint2 *>(p + 16) = make_uint2(v.z, v.w);
        }
    }
}
__device__ __forceinline__ void nlr_load_bt(const __bf16 *base, uint32_t ld, uint32_t s0, uint32_t M, int col, int q, uint32_t c0, BT<2> &t) {
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const uint32_t smp = s0 + 16 * n + col;
        const uint32_t sc = smp < M ? smp : M - 1;
        const __bf16 *p = base + (size_t)sc * ld + c0 + 4 * q;
        const uint2 a = *reinterpret_cast<const uint2 *>(p), b = *reinterpret_cast<const uint2 *>(p + 16);
        t.n[n] = __builtin_bit_cast(bf16x8, make_uint4(a.x, a.y, b.x, b.y));
    }
}
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// gradient piece P (as nlr_pack_piece) masked by the saved post-ReLU activation: x > 0 <=> its bf16 bits are non-zero
template <int P>
__device__ __forceinline__ void nlr_pack_masked(BT<2> &dst, const Unit<2> &src, const BT<2> &act) {
    constexpr int n = P >> 2, jb = (P >> 1) & 1, pr = P & 1;
    const f32x2 x = {src.a[jb][n][2 * pr], src.a[jb][n][2 * pr + 1]};
    const bf16x2 v = __builtin_convertvector(x, bf16x2);
    const u32x4 av = __builtin_bit_cast(u32x4, act.n[n]);
    const uint32_t ab = av[2 * jb + pr];
    const uint32_t m = ((ab & 0xffffu) ? 0xffffu : 0u) | ((ab & 0xffff0000u) ? 0xffff0000u : 0u);
    const uint32_t r = __builtin_bit_cast(uint32_t, v) & m;
    const bf16x2 o = __builtin_bit_cast(bf16x2, r);
    dst.n[n][4 * jb + 2 * pr] = o[0];
    dst.n[n][4 * jb + 2 * pr + 1] = o[1];
}

__device__ __forceinline__ void nlr_zero(Unit<2> &u) {
#pragma unroll
    for (int jb = 0; jb < 2; ++jb)
#pragma unroll
        for (int n = 0; n < 2; ++n) u.a[jb][n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

// WT = view width / 32, BW = bottleneck / 32, FT = ceil(F / 32), HT = head hidden units of 32 (0, 2, 4)
// VIEW = false: rows without colour supervision (nlr_mlp_train_*_split): density trunk and heads only, on the tapes
//   forward D0 D2 [H1 H2], backward H2^T [H1^T | e_0] D2^T D0^T; rgb is written as 0, the view columns of acts / gacts and the
//   rgb_layer columns of gacts are neither read nor written.  WT does not enter these instances.
template <int WT, int BW, int FT, int HT, bool BWD, bool VIEW = true>
__global__ void __launch_bounds__(256, 1) nlr_mlp_train_kernel(TrainParams P) {
    __shared__ __align__(16) uint4 lds_tape[NLR_NBUF * NLR_CHUNK_SLOTS];
    __shared__ __align__(16) float lds_bias[NLR_BIAS_MAX];
    __shared__ uint32_t lds_sig;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, q = lane >> 4;
    constexpr int HTA = HT > 0 ? HT : 1;
    // the forward and backward programs on the tapes and the offsets of the bias block (nlr_tape.h; plan_build checks against the same table)
    constexpr TrainProgram PG = nlr_train_program(WT, BW, FT, HT, VIEW);
    constexpr int VW = VIEW ? WT : 0;  // k-blocks of view gradients in BIG
    static_assert(PG.FR_HL % NLR_CHUNK_FRAGS == 0, "hidden view layers must cover whole chunks");
    // columns of acts / gacts (the depth is a run-time value: the two blocks behind the view layers are placed from P.act_w)
    constexpr TrainCols CC = nlr_train_cols(WT * 32, BW * 32, HT, 0);
    constexpr uint32_t C_HID = CC.c_hid, C_HBE = CC.c_hbe, C_Q = CC.c_q, C_X = CC.c_x;
    const uint32_t W = WT * 32, ld = P.act_w, gld = P.act_w + 64, C_LO = P.act_w, C_O = P.act_w + 32;

    const uint32_t ntiles = (P.M - P.row0 + 127) / 128;
    if (!BWD)
        for (uint32_t i = threadIdx.x * 4; i < P.bias_count; i += 1024)
            *reinterpret_cast<f32x4 *>(lds_bias + i) = *reinterpret_cast<const f32x4 *>(P.bias_all + i);
    Tape tp;
    tp.base = P.tape;
    tp.lds = lds_tape;
    tp.sig = &lds_sig;
    tp.sig_addr = (uint32_t)(uintptr_t)(nlr_lptr)&lds_sig;
    tp.total = (int)P.tape_chunks;
    tp.tid = threadIdx.x;
    tp.lane = lane;
    tp.prologue();

    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    auto bias_rows = [&](const float *b, f32x4 (&out)[2]) {
        out[0] = *reinterpret_cast<const f32x4 *>(b + 4 * q);
        out[1] = *reinterpret_cast<const f32x4 *>(b + 16 + 4 * q);
    };
    auto no_bias = [&](auto, f32x4 (&out)[2]) { out[0] = out[1] = zero4; };
    // ---- the recurring callbacks of nlr_gemm
    // bias: the rows of output unit O from the block at lds_bias + OB (OB: a constant as ic<>)
    auto bias_at = [&](auto ob) {
        return [&](auto o, f32x4(&out)[2]) { bias_rows(lds_bias + decltype(ob)::value + 32 * decltype(o)::value, out); };
    };
    // mma: one accumulator chain over the B tiles t[0 .. KG)
    auto chain = [](const BT<2> *t) {
        return [t](Unit<2> &u, auto g, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
            constexpr int G = decltype(g)::value, J = decltype(j)::value;
            nlr_mma_bf16<G == 0, 0>(u.a[J], bj, f0, t[G]);
        };
    };

    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t s0 = P.row0 + tile * 128 + wave * 32;
        if constexpr (!BWD) {
            // ======================================================= forward =======================================================
            BT<2> fb[FT], hbe[BW + 1];
            {
                Unit<2> fin, eu;
#pragma unroll
                for (int t = 0; t < FT; ++t) {
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        const uint32_t smp = s0 + 16 * n + col, sc = smp < P.M ? smp : P.M - 1;
#pragma unroll
                        for (int jb = 0; jb < 2; ++jb) {
                            const uint32_t f0 = 32 * t + 16 * jb + 4 * q;
                            fin.a[jb][n] = f0 + 4 <= P.F ? *reinterpret_cast<const f32x4 *>(P.feat + (size_t)sc * P.F + f0) : zero4;
                        }
                    }
                    nlr_pack_all<false, 0>(fb[t], fin);
                }
                if constexpr (VIEW) {
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        const uint32_t smp = s0 + 16 * n + col, sc = smp < P.M ? smp : P.M - 1;
#pragma unroll
                        for (int jb = 0; jb < 2; ++jb) eu.a[jb][n] = *reinterpret_cast<const f32x4 *>(P.enc + (size_t)(sc / P.S) * 32 + 16 * jb + 4 * q);
                    }
                    nlr_pack_all<false, 0>(hbe[BW], eu);
                }
            }
            BT<2> hidb[2];
            nlr_gemm<2, FT, 2, 2, 1, 0, 9>(
                tp, bias_at(ic<PG.OB_D0>{}),
                chain(fb),
                [&](auto o, auto p, const Unit<2> &u) {
                    constexpr int O = decltype(o)::value, Pc = decltype(p)::value;
                    if constexpr (Pc < 8) nlr_pack_piece<true, Pc, 0>(hidb[O], u);
                    else nlr_store_bt(P.acts, ld, s0, P.M, col, q, C_HID + 32 * O, hidb[O]);
                });
            float raw[2] = {0.0f, 0.0f};
            nlr_gemm<BW, 2, 2, 2, 1, PG.FR_D0, 9>(
                tp, bias_at(ic<PG.OB_D2>{}),
                chain(hidb),
                [&](auto o, auto p, const Unit<2> &u) {
                    constexpr int O = decltype(o)::value, Pc = decltype(p)::value;
                    if constexpr (O == 0 && Pc == 0) {
                        raw[0] = u.a[0][0][0];
                        raw[1] = u.a[0][1][0];
                    }
                    if constexpr (Pc < 8) nlr_pack_piece<false, Pc, 0>(hbe[O], u);
                    else nlr_store_bt(P.acts, ld, s0, P.M, col, q, C_HBE + 32 * O, hbe[O]);
                });
            Unit<2> lo;
            nlr_zero(lo);
            if constexpr (HT > 0) {
                BT<2> qb[HTA];
                nlr_gemm<HT, BW, 2, 2, 1, PG.FR_D0 + PG.FR_D2, 9>(
                    tp, bias_at(ic<PG.OB_H1>{}),
                    chain(hbe),
                    [&](auto o, auto p, const Unit<2> &u) {
                        constexpr int O = decltype(o)::value, Pc = decltype(p)::value;
                        if constexpr (Pc < 8) nlr_pack_piece<true, Pc, 0>(qb[O], u);
                        else nlr_store_bt(P.acts, ld, s0, P.M, col, q, C_Q + 32 * O, qb[O]);
                    });
                nlr_gemm<1, HT, 2, 2, 1, PG.FR_D0 + PG.FR_D2 + PG.FR_H1, 1>(
                    tp, bias_at(ic<PG.OB_H2>{}),
                    chain(qb),
                    [&](auto, auto, const Unit<2> &u) { lo = u; });
            }
            // per-sample heads (layouts of the inference kernel)
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const uint32_t smp = s0 + 16 * n + col;
                const bool valid = smp < P.M;
                if (q == 0 && valid) {
                    P.density[smp] = nlr_softplus(raw[n] + P.density_bias);
                }
                if constexpr (HT > 0) {
                    if (P.K > 0) {
                        float e[2][4], mx = -INFINITY, s = 0.0f;
#pragma unroll
                        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                e[jb][r] = (16 * jb + 4 * q + r) < (int)P.K ? lo.a[jb][n][r] : -INFINITY;
                                mx = fmaxf(mx, e[jb][r]);
                            }
                        mx = nlr_q_max(mx);
#pragma unroll
                        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                e[jb][r] = expf(e[jb][r] - mx);
                                s += e[jb][r];
                            }
                        s = nlr_q_sum(s);
#pragma unroll
                        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int row = 16 * jb + 4 * q + r;
                                if (valid && row < (int)P.K) P.sem[(size_t)row * P.ldm + smp] = e[jb][r] / s;
                            }
                    }
                    if (P.inten && valid) {
#pragma unroll
                        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (16 * jb + 4 * q + r == (int)P.int_row) P.inten[smp] = lo.a[jb][n][r];
                    }
                }
            }
            if constexpr (!VIEW) {
                // no colour supervision: rgb = 0 (the compositing operator reads it), the view columns of acts stay unwritten
                if (q == 0) {
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        const uint32_t smp = s0 + 16 * n + col;
                        if (smp < P.M) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) P.rgb[(size_t)c * P.ldm + smp] = 0.0f;
                        }
                    }
                }
                nlr_pad<PG.FR_T % NLR_CHUNK_FRAGS>(tp);
            } else {
                // view MLP
                BT<2> x[WT], y[WT];
                nlr_gemm<WT, BW + 1, 2, 2, 1, PG.FR_T, 9>(
                    tp, bias_at(ic<PG.OB_V0>{}),
                    chain(hbe),
                    [&](auto o, auto p, const Unit<2> &u) {
                        constexpr int O = decltype(o)::value, Pc = decltype(p)::value;
                        if constexpr (Pc < 8) nlr_pack_piece<true, Pc, 0>(x[O], u);
                        else nlr_store_bt(P.acts, ld, s0, P.M, col, q, C_X + 32 * O, x[O]);
                    });
                nlr_gemm<WT, WT + BW + 1, 2, 2, 1, PG.FR_T + PG.FR_V0, 9>(
                    tp, bias_at(ic<PG.OB_V1>{}),
                    [&](Unit<2> &u, auto g, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
                        constexpr int G = decltype(g)::value, J = decltype(j)::value;
                        if constexpr (G < WT) nlr_mma_bf16<G == 0, 0>(u.a[J], bj, f0, x[G]);
                        else nlr_mma_bf16<false, 0>(u.a[J], bj, f0, hbe[G - WT]);
                    },
                    [&](auto o, auto p, const Unit<2> &u) {
                        constexpr int O = decltype(o)::value, Pc = decltype(p)::value;
                        if constexpr (Pc < 8) nlr_pack_piece<true, Pc, 0>(y[O], u);
                        else nlr_store_bt(P.acts, ld, s0, P.M, col, q, C_X + W + 32 * O, y[O]);
                    });
                for (uint32_t l = 2; l < P.depth; ++l) {
                    const float *bl = lds_bias + PG.OB_VL + (l - 2) * (WT * 32);
                    const uint32_t cl = C_X + l * W;
                    nlr_gemm<WT, WT, 2, 2, 1, PG.FF_HID, 9>(
                        tp, [&](auto o, f32x4(&b)[2]) { bias_rows(bl + 32 * decltype(o)::value, b); },
                        chain(y),
                        [&](auto o, auto p, const Unit<2> &u) {
                            constexpr int O = decltype(o)::value, Pc = decltype(p)::value;
                            if constexpr (Pc < 8) nlr_pack_piece<true, Pc, 0>(x[O], u);
                            else nlr_store_bt(P.acts, ld, s0, P.M, col, q, cl + 32 * O, x[O]);
                        });
#pragma unroll
                    for (int t = 0; t < WT; ++t) y[t] = x[t];
                }
                Unit<2> out1;
                nlr_gemm<1, WT, 1, 2, 1, PG.FF_HID, 1>(
                    tp, [&](auto, f32x4(&b)[2]) { bias_rows(lds_bias + PG.OB_VL + (P.depth - 2) * (WT * 32), b); },
                    chain(y),
                    [&](auto, auto, const Unit<2> &u) { out1 = u; });
                if (q == 0) {
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        const uint32_t smp = s0 + 16 * n + col;
                        if (smp < P.M) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                const float z = P.rgb_premul * out1.a[0][n][c] + P.rgb_bias;
                                const float sg = 1.0f / (1.0f + expf(-z));
                                P.rgb[(size_t)c * P.ldm + smp] = sg * (1.0f + 2.0f * P.rgb_padding) - P.rgb_padding;
                            }
                        }
                    }
                }
                nlr_pad<PG.FF_END % NLR_CHUNK_FRAGS>(tp);
            }
        } else {
            // ======================================================= backward ======================================================
            // d loss / d (rgb_layer output): rgb = s (1 + 2p) - p, s = sigmoid(premul o + bias)
            BT<2> gin;  // one 32-feature k-block of upstream gradient
            BT<2> g[WT], h[WT], mk;
            // epi: the gradient of a ReLU layer's pre-activation: unit O masked by the saved activation at columns c0 + 32 O of acts,
            // packed into dst[O] and stored at the same columns of gacts
            auto mask_store = [&](BT<2> *dst, uint32_t c0) {
                return [&, dst, c0](auto o, auto p, const Unit<2> &u) {
                    constexpr int O = decltype(o)::value, Pc = decltype(p)::value;
                    if constexpr (Pc == 0) nlr_load_bt(P.acts, ld, s0, P.M, col, q, c0 + 32 * O, mk);
                    if constexpr (Pc < 8) nlr_pack_masked<Pc>(dst[O], u, mk);
                    else nlr_store_bt(P.gacts, gld, s0, P.M, col, q, c0 + 32 * O, dst[O]);
                };
            };
            if constexpr (VIEW) {
                {
                    Unit<2> du;
                    nlr_zero(du);
                    if (q == 0 && P.g_rgb) {
#pragma unroll
                        for (int n = 0; n < 2; ++n) {
                            const uint32_t smp = s0 + 16 * n + col;
                            if (smp < P.M) {
#pragma unroll
                                for (int c = 0; c < 3; ++c) {
                                    const float s = (P.rgb[(size_t)c * P.ldm + smp] + P.rgb_padding) / (1.0f + 2.0f * P.rgb_padding);
                                    du.a[0][n][c] = P.g_rgb[(size_t)c * P.ldm + smp] * (1.0f + 2.0f * P.rgb_padding) * (s * (1.0f - s)) * P.rgb_premul;
                                }
                            }
                        }
                    }
                    nlr_pack_all<false, 0>(gin, du);
                    nlr_store_bt(P.gacts, gld, s0, P.M, col, q, C_O, gin);
                }
                {  // RGB^T: gradient of the last view layer's pre-activation
                    const uint32_t cl = C_X + (P.depth - 1) * W;
                    nlr_gemm<WT, 1, 2, 2, 1, 0, 9>(
                        tp, no_bias,
                        chain(&gin),
                        mask_store(g, cl));
                }
                for (uint32_t l = P.depth - 1; l >= 2; --l) {  // hidden layers, transposed: d z_{l-1} = mask(x_{l-1}) W_l^T d z_l
                    const uint32_t cl = C_X + (l - 1) * W;
                    nlr_gemm<WT, WT, 2, 2, 1, PG.BR_RGB, 9>(
                        tp, no_bias,
                        chain(g),
                        mask_store(h, cl));
#pragma unroll
                    for (int t = 0; t < WT; ++t) g[t] = h[t];
                }
                // g = d z_1.  V1a^T: d z_0 = mask(x_0) W1[:, :W]^T d z_1
                nlr_gemm<WT, WT, 2, 2, 1, PG.BF_V1A, 9>(
                    tp, no_bias,
                    chain(g),
                    mask_store(h, C_X));
            }
            // heads: softmax backward d l_c = p_c (g_c - sum_k g_k p_k), intensity row: its upstream gradient
            BT<2> gq[HTA], aux;
            {
                Unit<2> dl, da;
#pragma unroll
                for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                    for (int n = 0; n < 2; ++n) dl.a[jb][n] = da.a[jb][n] = zero4;
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const uint32_t smp = s0 + 16 * n + col;
                    const bool valid = smp < P.M;
                    if constexpr (HT > 0) {
                        if (P.K > 0 && P.g_sem) {
                            float pr[2][4], gr[2][4], dot = 0.0f;
#pragma unroll
                            for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const int row = 16 * jb + 4 * q + r;
                                    const bool on = valid && row < (int)P.K;
                                    pr[jb][r] = on ? P.sem[(size_t)row * P.ldm + smp] : 0.0f;
                                    gr[jb][r] = on ? P.g_sem[(size_t)row * P.ldm + smp] : 0.0f;
                                    dot += pr[jb][r] * gr[jb][r];
                                }
                            dot = nlr_q_sum(dot);
#pragma unroll
                            for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                                for (int r = 0; r < 4; ++r) dl.a[jb][n][r] = pr[jb][r] * (gr[jb][r] - dot);
                        }
                        if (P.g_inten && valid) {
#pragma unroll
                            for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                                for (int r = 0; r < 4; ++r)
                                    if (16 * jb + 4 * q + r == (int)P.int_row) dl.a[jb][n][r] = P.g_inten[smp];
                        }
                    }
                    // raw density: density = softplus(raw + bias) -> d raw = g (1 - exp(-density)); fed to BIG as two bf16 features
                    // (hi + lo) with unit weights on bottleneck row 0
                    if (q == 0 && valid && P.g_density) {
                        const float dr = P.g_density[smp] * (1.0f - expf(-P.density[smp]));
                        const float hi = (float)(__bf16)dr;
                        da.a[0][n][0] = hi;
                        da.a[0][n][1] = dr - hi;
                    }
                }
                nlr_pack_all<false, 0>(gin, dl);
                nlr_store_bt(P.gacts, gld, s0, P.M, col, q, C_LO, gin);
                nlr_pack_all<false, 0>(aux, da);
            }
            if constexpr (HT > 0) {  // H2^T: d (head hidden pre-activation)
                nlr_gemm<HT, 1, 2, 2, 1, PG.BF_H2, 9>(
                    tp, no_bias,
                    chain(&gin),
                    mask_store(gq, C_Q));
            }
            // BIG: d bottleneck = W1[:, W:W+WB]^T d z_1 + W0[:, :WB]^T d z_0 + H1^T d q + e_0 d raw (without the view MLP: the last two)
            BT<2> gb[BW];
            nlr_gemm<BW, 2 * VW + HT + 1, 2, 2, 1, PG.BF_BIG, 9>(
                tp, no_bias,
                [&](Unit<2> &u, auto gg, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
                    constexpr int G = decltype(gg)::value, J = decltype(j)::value;
                    if constexpr (G < VW) nlr_mma_bf16<G == 0, 0>(u.a[J], bj, f0, g[G]);
                    else if constexpr (G < 2 * VW) nlr_mma_bf16<false, 0>(u.a[J], bj, f0, h[G - VW]);
                    else if constexpr (G < 2 * VW + HT) nlr_mma_bf16<G == 0, 0>(u.a[J], bj, f0, gq[G - 2 * VW]);
                    else nlr_mma_bf16<G == 0, 0>(u.a[J], bj, f0, aux);
                },
                [&](auto o, auto p, const Unit<2> &u) {
                    constexpr int O = decltype(o)::value, Pc = decltype(p)::value;
                    if constexpr (Pc < 8) nlr_pack_piece<false, Pc, 0>(gb[O], u);
                    else nlr_store_bt(P.gacts, gld, s0, P.M, col, q, C_HBE + 32 * O, gb[O]);
                });
            // D2^T: d (trunk hidden pre-activation)
            BT<2> gh[2];
            nlr_gemm<2, BW, 2, 2, 1, PG.BF_D2, 9>(
                tp, no_bias,
                chain(gb),
                mask_store(gh, C_HID));
            // D0^T: gradient of the grid features, f32 out
            nlr_gemm<FT, 2, 2, 2, 1, PG.BF_D0, 1>(
                tp, no_bias,
                chain(gh),
                [&](auto o, auto, const Unit<2> &u) {
                    constexpr int O = decltype(o)::value;
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        const uint32_t smp = s0 + 16 * n + col;
#pragma unroll
                        for (int jb = 0; jb < 2; ++jb) {
                            const uint32_t f0 = 32 * O + 16 * jb + 4 * q;
                            if (smp < P.M && f0 + 4 <= P.F) *reinterpret_cast<f32x4 *>(P.d_feat + (size_t)smp * P.F + f0) = u.a[jb][n];
                        }
                    }
                });
            nlr_pad<PG.BF_END % NLR_CHUNK_FRAGS>(tp);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- device-side tape packing: tape element i (bf16) = flat parameter idx[i] (or 0 when idx[i] < 0); bias block likewise in f32
__global__ void __launch_bounds__(256) nlr_train_pack_kernel(const float *__restrict__ params, const int32_t *__restrict__ idx, uint32_t n,
                                                            __bf16 *__restrict__ tape, const int32_t *__restrict__ bidx, uint32_t nb,
                                                            float *__restrict__ bias) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const int32_t k = idx[i];  // -1: structural zero, -2: structural one
        tape[i] = k >= 0 ? (__bf16)params[k] : (k == -2 ? (__bf16)1.0f : (__bf16)0.0f);
    }
    if (i < nb) {
        const int32_t k = bidx[i];
        bias[i] = k >= 0 ? params[k] : 0.0f;
    }
}

// ---- plan: shapes, parameter order, index maps ----------------------------------------------------------------------------------
typedef TapeMat<int32_t, -1> IMat;  // matrix of flat-parameter indices (-1 = structural zero)
typedef TapeLinear<int32_t, -1> ILin;
// one GEMM on an index tape: the walk of the weight tapes (nlr_tape.h) over indices, bf16 k-groups
static void tape_add(std::vector<int32_t> &t, const IMat &w, uint32_t out_pad, uint32_t in_pad, uint32_t RH = 2) {
    nlr_tape_walk(w, out_pad, in_pad, 32, RH, [&](const int32_t *v, uint32_t n) { t.insert(t.end(), v, v + n); });
}
static void tape_pad(std::vector<int32_t> &t) { t.resize((t.size() + NLR_CHUNK_BF16 - 1) / NLR_CHUNK_BF16 * NLR_CHUNK_BF16, -1); }

// Everything of a plan that needs no device: the scalars, the layer table and the index maps of the two tapes and of the bias block.
// Flat parameter order (weights row-major [out, in], then bias), one TrainLinear each:
//   density_layer.0, density_layer.2, [sem_layer.0, sem_layer.2], [intensity_layer.0, intensity_layer.2], lin_second_stage_0..D-1, rgb_layer
static int plan_build(NlrTrainPlan *p, uint32_t F, uint32_t W, uint32_t WB, uint32_t D, uint32_t deg_view, uint32_t class_num,
                      int use_semantic, int use_intensity, std::vector<int32_t> &ft, std::vector<int32_t> &bt, std::vector<int32_t> &bb) {
    const uint32_t E = 3 + 6 * deg_view;
    p->F = F, p->W = W, p->WB = WB, p->D = D, p->E = E, p->sem = use_semantic != 0, p->inten = use_intensity != 0;
    const uint32_t K = p->K = p->sem ? class_num : 0;
    p->int_row = p->inten ? K : 0xffffffffu;
    p->HT = (p->sem ? 2 : 0) + (p->inten ? 2 : 0);
    const TrainCols c = nlr_train_cols(W, WB, p->HT, D);
    p->act_w = c.c_lo;
    // ---- the layer table; each entry takes its weight and bias from the flat buffer
    uint32_t off = 0;
    auto add = [&](uint32_t g_col, uint32_t o_off, uint32_t n_out, uint32_t color, std::initializer_list<TrainBlock> in) {
        TrainLinear l = {};
        l.g_col = g_col, l.o_off = o_off, l.n_out = n_out, l.color = color;
        uint32_t cols = 0;
        for (const TrainBlock &k : in) l.in[l.n_in++] = k, cols += k.n;
        l.w_off = off, l.b_off = off + n_out * cols;
        off = l.b_off + n_out;
        p->linears.push_back(l);
        ILin x;
        x.w = IMat(n_out, cols);
        for (size_t i = 0; i < x.w.a.size(); ++i) x.w.a[i] = (int32_t)(l.w_off + i);
        for (uint32_t i = 0; i < n_out; ++i) x.b.push_back((int32_t)(l.b_off + i));
        return x;
    };
    const TrainBlock hbe = {NLR_TRAIN_SRC_ACTS, c.c_hbe, WB}, encb = {NLR_TRAIN_SRC_ENC, 0, E};
    auto acts = [](uint32_t col, uint32_t n) { return TrainBlock{NLR_TRAIN_SRC_ACTS, col, n}; };
    ILin s0, s2, i0, i2;
    std::vector<ILin> v(D);
    const ILin d0 = add(c.c_hid, 0, 64, 0, {{NLR_TRAIN_SRC_FEATURES, 0, F}});
    const ILin d2 = add(c.c_hbe, 0, WB, 0, {acts(c.c_hid, 64)});
    uint32_t r0 = 0;  // head hidden units: [sem 64][intensity 64]
    if (p->sem) {
        s0 = add(c.c_q, 0, 64, 0, {hbe});
        s2 = add(c.c_lo, 0, K, 0, {acts(c.c_q, 64)});
        r0 = 64;
    }
    if (p->inten) {
        i0 = add(c.c_q + r0, 0, 64, 0, {hbe});
        i2 = add(c.c_lo + K, K, 1, 0, {acts(c.c_q + r0, 64)});
    }
    v[0] = add(c.c_x, 0, W, 1, {hbe, encb});
    v[1] = add(c.c_x + W, 0, W, 1, {acts(c.c_x, W), hbe, encb});  // the skip concatenation
    for (uint32_t l = 2; l < D; ++l) v[l] = add(c.c_x + l * W, 0, W, 1, {acts(c.c_x + (l - 1) * W, W)});
    const ILin rgb = add(c.c_o, 0, 3, 1, {acts(c.c_x + (D - 1) * W, W)});
    p->n_params = off;
    // heads as two stacked GEMMs, as the inference path
    const TapeHeads<int32_t, -1> hd = nlr_tape_heads<int32_t, -1>(WB, K, p->sem ? &s0 : nullptr, &s2, p->inten ? &i0 : nullptr, &i2);
    const uint32_t HH = p->HT * 32, Fp = 64;  // (grid features padded to two k-blocks)
    // view layers with the direction-encoding columns padded to one 32-feature k-block
    const IMat v0p = v[0].w.slice(0, W, 0, WB + 32), v1p = v[1].w.slice(0, W, 0, W + WB + 32);
    // ---- the tapes: forward D0 D2 [H1 H2] (V0 V1 L2.. RGB), backward (RGB^T L^T.. V1a^T) H2^T BIG D2^T D0^T; the parts in brackets
    //      with the view MLP only.  Each program's length is checked against the kernel's (nlr_train_program).
    auto build_tapes = [&](bool view) -> int {
        const TrainProgram PG = nlr_train_program(W / 32, WB / 32, Fp / 32, p->HT, view);
        const size_t f_start = ft.size(), b_start = bt.size(), frag = NLR_FRAG_BYTES / 2;  // (bf16 elements per fragment)
        tape_add(ft, d0.w, 64, Fp);
        tape_add(ft, d2.w, WB, 64);
        if (HH) {
            tape_add(ft, hd.h1, HH, WB);
            tape_add(ft, hd.h2, 32, HH);
        }
        if (view) {
            tape_add(ft, v0p, W, WB + 32);
            tape_add(ft, v1p, W, W + WB + 32);
            for (uint32_t l = 2; l < D; ++l) tape_add(ft, v[l].w, W, W);
            tape_add(ft, rgb.w, 16, W, 1);
        }
        if (const int rc = nlr_tape_check(view ? "training forward tape (fragments)" : "training forward tape, trunk and heads (fragments)",
                                          (ft.size() - f_start) / frag, PG.fwd_frags(D)))
            return rc;
        tape_pad(ft);
        const uint32_t VW = view ? W : 0;
        if (view) {
            tape_add(bt, rgb.w.t(), W, 32);  // rows = view features, k = the 3 (of 32) rgb rows
            for (uint32_t l = D - 1; l >= 2; --l) tape_add(bt, v[l].w.t(), W, W);
            tape_add(bt, v[1].w.slice(0, W, 0, W).t(), W, W);  // V1a^T: d z_0 <- d z_1 through W1[:, :W]
        }
        if (HH) tape_add(bt, hd.h2.t(), HH, 32);
        IMat big(WB, 2 * VW + HH + 32);
        big.paste(0, 0, v[1].w.slice(0, VW, W, WB).t());  // skip concat of layer 1
        big.paste(0, VW, v[0].w.slice(0, VW, 0, WB).t());  // layer 0
        big.paste(0, 2 * VW, hd.h1.t());                   // heads
        big.at(0, 2 * VW + HH + 0) = -2;  // unit weights: raw-density gradient (hi, lo) onto bottleneck row 0
        big.at(0, 2 * VW + HH + 1) = -2;
        tape_add(bt, big, WB, 2 * VW + HH + 32);
        tape_add(bt, d2.w.t(), 64, WB);
        tape_add(bt, d0.w.t(), Fp, 64);
        if (const int rc = nlr_tape_check(view ? "training backward tape (fragments)" : "training backward tape, trunk and heads (fragments)",
                                          (bt.size() - b_start) / frag, PG.bwd_frags(D)))
            return rc;
        tape_pad(bt);
        return NLR_OK;
    };
    if (const int rc = build_tapes(true)) return rc;
    // the tapes of rows without colour supervision (nlr_mlp_train_*_split) behind the full ones, so that one gather packs both
    p->f0n = p->f1 = (uint32_t)ft.size(), p->b0n = p->b1 = (uint32_t)bt.size();
    if (const int rc = build_tapes(false)) return rc;
    p->fn = (uint32_t)ft.size(), p->bn = (uint32_t)bt.size();
    p->f1n = p->fn - p->f1, p->b1n = p->bn - p->b1;
    // ---- bias block of the forward kernel (order: nlr_tape.h)
    auto pushb = [&](const std::vector<int32_t> &b, uint32_t pad) {
        bb.insert(bb.end(), b.begin(), b.end());
        bb.resize(bb.size() + pad - b.size(), -1);
    };
    pushb(d0.b, 64);
    pushb(d2.b, WB);
    pushb(hd.b1, HH);
    pushb(hd.b2, 32);
    for (uint32_t l = 0; l < D; ++l) pushb(v[l].b, W);
    pushb(rgb.b, 32);
    p->biasn = (uint32_t)bb.size();
    return nlr_tape_check("training bias block (floats)", bb.size(), nlr_train_program(W / 32, WB / 32, Fp / 32, p->HT, true).bias_end(D));
}

// the device side of a plan; on failure the caller destroys the plan with what it owns by then
static int plan_upload(NlrTrainPlan *p, const std::vector<int32_t> &ft, const std::vector<int32_t> &bt, const std::vector<int32_t> &bb) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        NLR_FAIL(NLR_ERR_HIP, "train_plan_create: cannot query the current device");
    p->cus = (uint32_t)cus;
    NLR_CHECK_ARG(p->biasn <= NLR_BIAS_MAX && p->biasn % 4 == 0, "train_plan_create: bias block of %u floats does not fit", p->biasn);
    auto up = [&](const std::vector<int32_t> &h, int32_t **d) -> int {
        NLR_HIP(hipMalloc((void **)d, h.size() * 4));
        NLR_HIP(hipMemcpy(*d, h.data(), h.size() * 4, hipMemcpyHostToDevice));
        return NLR_OK;
    };
    int rc;
    if ((rc = up(ft, &p->fidx)) || (rc = up(bt, &p->bidx)) || (rc = up(bb, &p->biasidx))) return rc;
    const size_t slack = NLR_TAPE_SLACK_CHUNKS * NLR_CHUNK_BF16;  // the kernel prefetches past the end
    NLR_HIP(hipMalloc((void **)&p->ftape, (ft.size() + slack) * 2));
    NLR_HIP(hipMalloc((void **)&p->btape, (bt.size() + slack) * 2));
    NLR_HIP(hipMemset(p->ftape, 0, (ft.size() + slack) * 2));
    NLR_HIP(hipMemset(p->btape, 0, (bt.size() + slack) * 2));
    NLR_HIP(hipMalloc((void **)&p->bias, bb.size() * 4));
    return NLR_OK;
}

extern "C" void nlr_train_plan_destroy(NlrTrainPlan *p) {
    if (!p) return;
    (void)hipFree(p->fidx), (void)hipFree(p->bidx), (void)hipFree(p->biasidx), (void)hipFree(p->ftape), (void)hipFree(p->btape), (void)hipFree(p->bias);
    delete p;
}

extern "C" int nlr_train_plan_create(uint32_t F, uint32_t W, uint32_t WB, uint32_t D, uint32_t deg_view, uint32_t class_num, int use_semantic,
                                     int use_intensity, float density_bias, float rgb_premultiplier, float rgb_bias, float rgb_padding,
                                     NlrTrainPlan **out, uint32_t *n_params) {
    NLR_CHECK_ARG(out && n_params, "train_plan_create: NULL argument");
    NLR_CHECK_ARG(WB == 256 && (W == 128 || W == 256) && F % 4 == 0 && F > 32 && F <= 64 && D >= 2 && D <= 10 && 3 + 6 * deg_view <= 32 &&
                      class_num <= 31,
                  "train_plan_create: unsupported NerfMLP shape (bottleneck 256, view width 128/256, 33..64 grid features, depth 2..10)");
    NlrTrainPlan *p = new NlrTrainPlan();
    p->density_bias = density_bias, p->rgb_premul = rgb_premultiplier, p->rgb_bias = rgb_bias, p->rgb_padding = rgb_padding;
    std::vector<int32_t> ft, bt, bb;
    int rc = plan_build(p, F, W, WB, D, deg_view, class_num, use_semantic, use_intensity, ft, bt, bb);
    if (!rc) rc = plan_upload(p, ft, bt, bb);
    if (rc) {
        nlr_train_plan_destroy(p);
        return rc;
    }
    *out = p;
    *n_params = p->n_params;
    return NLR_OK;
}

extern "C" uint32_t nlr_train_act_width(const NlrTrainPlan *p) { return p ? p->act_w : 0; }

// offsets (in floats) of every (weight, bias) pair inside the flat parameter buffer, in the order documented above
extern "C" int nlr_train_param_layout(const NlrTrainPlan *p, uint32_t *offsets, uint32_t capacity) {
    NLR_CHECK_ARG(p && offsets && capacity >= 2 * p->linears.size(), "train_param_layout: buffer too small (%zu entries)",
                  p ? 2 * p->linears.size() : 0);
    for (size_t i = 0; i < p->linears.size(); ++i) offsets[2 * i] = p->linears[i].w_off, offsets[2 * i + 1] = p->linears[i].b_off;
    return (int)(2 * p->linears.size());
}

// the layer table, NLR_TRAIN_TABLE_ROW uint32 per Linear (header section 6b); returns the number of rows
extern "C" int nlr_train_linear_table(const NlrTrainPlan *p, uint32_t *rows, uint32_t capacity) {
    NLR_CHECK_ARG(p && rows && capacity >= NLR_TRAIN_TABLE_ROW * p->linears.size(), "train_linear_table: buffer too small (%zu entries)",
                  p ? NLR_TRAIN_TABLE_ROW * p->linears.size() : 0);
    for (const TrainLinear &l : p->linears) {
        *rows++ = l.g_col, *rows++ = l.o_off, *rows++ = l.n_out, *rows++ = l.color, *rows++ = l.n_in;
        for (const TrainBlock &k : l.in) *rows++ = k.src, *rows++ = k.col, *rows++ = k.n;
        *rows++ = l.w_off, *rows++ = l.b_off;
    }
    return (int)p->linears.size();
}

extern "C" int nlr_train_pack(NlrTrainPlan *p, const float *params_dev, void *stream) {
    NLR_CHECK_ARG(p && params_dev, "train_pack: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nlr_train_pack_kernel, dim3((p->fn + 255) / 256), dim3(256), 0, st, params_dev, p->fidx, p->fn, p->ftape, p->biasidx,
                       p->biasn, p->bias);
    hipLaunchKernelGGL(nlr_train_pack_kernel, dim3((p->bn + 255) / 256), dim3(256), 0, st, params_dev, p->bidx, p->bn, p->btape, nullptr, 0u,
                       nullptr);
    NLR_LAUNCH_CHECK("nlr_train_pack_kernel");
    return NLR_OK;
}

// VIEW = false: the trunk-and-heads instances, one per head count whatever the view width
template <bool BWD, bool VIEW>
static int launch_train(const NlrTrainPlan *p, TrainParams &P, hipStream_t st) {
    const uint32_t ntiles = (P.M - P.row0 + 127) / 128;
    dim3 grid(ntiles < p->cus ? ntiles : p->cus);
#define NLR_TR(wt, ht)                                                                                              \
    if ((!VIEW || p->W == wt * 32) && p->HT == ht) {                                                                \
        hipLaunchKernelGGL((nlr_mlp_train_kernel<VIEW ? wt : 4, 8, 2, ht, BWD, VIEW>), grid, dim3(256), 0, st, P);   \
        NLR_LAUNCH_CHECK(VIEW ? "nlr_mlp_train_kernel" : "nlr_mlp_train_kernel (trunk and heads)");                  \
        return NLR_OK;                                                                                              \
    }
    NLR_TR(8, 4) NLR_TR(8, 2) NLR_TR(8, 0) NLR_TR(4, 4) NLR_TR(4, 2) NLR_TR(4, 0)
#undef NLR_TR
    NLR_FAIL(NLR_ERR_UNSUPPORTED, "mlp_train: no kernel instance for view width %u with %u head units", p->W, p->HT);
}

static void fill_common(const NlrTrainPlan *p, TrainParams &P, uint32_t M, uint32_t S) {
    memset(&P, 0, sizeof(P));
    P.M = M, P.ldm = M, P.row0 = 0, P.S = S, P.F = p->F, P.depth = p->D, P.K = p->K, P.int_row = p->int_row, P.act_w = p->act_w;
    P.density_bias = p->density_bias, P.rgb_premul = p->rgb_premul, P.rgb_bias = p->rgb_bias, P.rgb_padding = p->rgb_padding;
}

// NLR_DBG_TRAIN_ROUTE / _TRUNK_ROW0 / _TRUNK_ROWS: which instances the last forward / backward call launched, and on which rows
static void note_route(bool bwd, uint32_t M, uint32_t M_color) {
    (void)nlr_debug_set(NLR_DBG_TRAIN_ROUTE, (M_color > 0 ? 1 : 0) | (M_color < M ? 2 : 0) | (bwd ? 4 : 0));
    (void)nlr_debug_set(NLR_DBG_TRAIN_TRUNK_ROW0, (int)M_color);
    (void)nlr_debug_set(NLR_DBG_TRAIN_TRUNK_ROWS, (int)(M - M_color));
}
// Rows [0, M_color) through the full instance, rows [M_color, M) through the trunk-and-heads instance: two launches on one stream.
template <bool BWD>
static int launch_rows(const NlrTrainPlan *p, TrainParams &P, uint32_t M, uint32_t M_color, hipStream_t st) {
    const __bf16 *tape = BWD ? p->btape : p->ftape;
    const uint32_t n0 = BWD ? p->b0n : p->f0n, t1 = BWD ? p->b1 : p->f1, n1 = BWD ? p->b1n : p->f1n;
    note_route(BWD, M, M_color);
    if (M_color > 0) {
        P.row0 = 0, P.M = M_color;
        P.tape = (const uint4 *)tape, P.tape_chunks = n0 / NLR_CHUNK_BF16;
        if (const int rc = launch_train<BWD, true>(p, P, st)) return rc;
    }
    if (M_color < M) {
        P.row0 = M_color, P.M = M;
        P.tape = (const uint4 *)(tape + t1), P.tape_chunks = n1 / NLR_CHUNK_BF16;
        if (const int rc = launch_train<BWD, false>(p, P, st)) return rc;
    }
    return NLR_OK;
}
#define NLR_CHECK_SPLIT(what)                                                                                                             \
    NLR_CHECK_ARG(M > 0, what ": M is 0");                                                                                                \
    NLR_CHECK_ARG(S > 0 && M % S == 0, what ": M = %u is not a multiple of S = %u (M %% S != 0)", M, S);                                  \
    NLR_CHECK_ARG(M_color <= M, what ": M_color = %u exceeds M = %u (M_color > M)", M_color, M);                                          \
    NLR_CHECK_ARG(M_color % S == 0, what ": M_color = %u is not a multiple of S = %u (M_color %% S != 0)", M_color, S)

// features [M, F] f32 row-major, enc [M / S, 32]; outputs as nlr_mlp_level; acts [M, act_w] bf16
static int train_forward(const NlrTrainPlan *p, const float *features, const float *enc, uint32_t M, uint32_t M_color, uint32_t S,
                         float *density, float *rgb, float *semantic, float *intensity, void *acts, void *stream) {
    TrainParams P;
    fill_common(p, P, M, S);
    P.feat = features, P.enc = enc;
    P.bias_all = p->bias, P.bias_count = p->biasn;
    P.density = density, P.rgb = rgb, P.sem = semantic, P.inten = p->inten ? intensity : nullptr;
    P.acts = (__bf16 *)acts;
    return launch_rows<false>(p, P, M, M_color, (hipStream_t)stream);
}

extern "C" int nlr_mlp_train_forward(const NlrTrainPlan *p, const float *features, const float *enc, uint32_t M, uint32_t S, float *density,
                                     float *rgb, float *semantic, float *intensity, void *acts, void *stream) {
    NLR_CHECK_ARG(p && features && enc && density && rgb && acts && M > 0 && S > 0, "mlp_train_forward: bad argument");
    NLR_CHECK_ARG((!p->sem || semantic) && (!p->inten || intensity), "mlp_train_forward: head output missing");
    return train_forward(p, features, enc, M, M, S, density, rgb, semantic, intensity, acts, stream);
}

extern "C" int nlr_mlp_train_forward_split(const NlrTrainPlan *p, const float *features, const float *enc, uint32_t M, uint32_t M_color,
                                           uint32_t S, float *density, float *rgb, float *semantic, float *intensity, void *acts,
                                           void *stream) {
    NLR_CHECK_ARG(p, "mlp_train_forward_split: plan is NULL");
    NLR_CHECK_ARG(features, "mlp_train_forward_split: features is NULL");
    NLR_CHECK_ARG(enc, "mlp_train_forward_split: enc is NULL");
    NLR_CHECK_ARG(density, "mlp_train_forward_split: density is NULL");
    NLR_CHECK_ARG(rgb, "mlp_train_forward_split: rgb is NULL");
    NLR_CHECK_ARG(acts, "mlp_train_forward_split: acts is NULL");
    NLR_CHECK_ARG(!p->sem || semantic, "mlp_train_forward_split: semantic is NULL");
    NLR_CHECK_ARG(!p->inten || intensity, "mlp_train_forward_split: intensity is NULL");
    NLR_CHECK_SPLIT("mlp_train_forward_split");
    return train_forward(p, features, enc, M, M_color, S, density, rgb, semantic, intensity, acts, stream);
}

// upstream gradients in the layouts of the outputs (any may be NULL); gacts [M, act_w + 64] bf16, d_features [M, F] f32
static int train_backward(const NlrTrainPlan *p, uint32_t M, uint32_t M_color, uint32_t S, const float *density, const float *rgb,
                          const float *semantic, const void *acts, const float *g_density, const float *g_rgb, const float *g_semantic,
                          const float *g_intensity, void *gacts, float *d_features, void *stream) {
    TrainParams P;
    fill_common(p, P, M, S);
    P.density = const_cast<float *>(density), P.rgb = const_cast<float *>(rgb), P.sem = const_cast<float *>(semantic);
    P.acts = (__bf16 *)const_cast<void *>(acts);
    P.g_density = g_density, P.g_rgb = g_rgb, P.g_sem = (p->sem && semantic) ? g_semantic : nullptr, P.g_inten = p->inten ? g_intensity : nullptr;
    P.gacts = (__bf16 *)gacts;
    P.d_feat = d_features;
    return launch_rows<true>(p, P, M, M_color, (hipStream_t)stream);
}

extern "C" int nlr_mlp_train_backward(const NlrTrainPlan *p, uint32_t M, uint32_t S, const float *density, const float *rgb, const float *semantic,
                                      const void *acts, const float *g_density, const float *g_rgb, const float *g_semantic,
                                      const float *g_intensity, void *gacts, float *d_features, void *stream) {
    NLR_CHECK_ARG(p && density && rgb && acts && gacts && d_features && M > 0 && S > 0, "mlp_train_backward: bad argument");
    return train_backward(p, M, M, S, density, rgb, semantic, acts, g_density, g_rgb, g_semantic, g_intensity, gacts, d_features, stream);
}

extern "C" int nlr_mlp_train_backward_split(const NlrTrainPlan *p, uint32_t M, uint32_t M_color, uint32_t S, const float *density,
                                            const float *rgb, const float *semantic, const void *acts, const float *g_density,
                                            const float *g_rgb, const float *g_semantic, const float *g_intensity, void *gacts,
                                            float *d_features, void *stream) {
    NLR_CHECK_ARG(p, "mlp_train_backward_split: plan is NULL");
    NLR_CHECK_ARG(density, "mlp_train_backward_split: density is NULL");
    NLR_CHECK_ARG(rgb, "mlp_train_backward_split: rgb is NULL");
    NLR_CHECK_ARG(acts, "mlp_train_backward_split: acts is NULL");
    NLR_CHECK_ARG(gacts, "mlp_train_backward_split: gacts is NULL");
    NLR_CHECK_ARG(d_features, "mlp_train_backward_split: d_features is NULL");
    NLR_CHECK_SPLIT("mlp_train_backward_split");
    return train_backward(p, M, M_color, S, density, rgb, semantic, acts, g_density, g_rgb, g_semantic, g_intensity, gacts, d_features, stream);
}
