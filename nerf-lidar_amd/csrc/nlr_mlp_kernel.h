// NerfMLP evaluation on the matrix cores: density trunk -> semantic/intensity heads -> view MLP -> rgb.
//
// Replaces (rows a-9..a-12 of the scope table):
//   ZI/models.py:887-889, 996-997, 1116     density_layer (F->64->256), softplus(raw - 1)
//   ZI/models.py:954-961, 1124-1143         sem_layer (256->64->19, softmax), intensity_layer (256->64->1)
//   ZI/coord.py:199-210, models.py:1190-1196  pos_enc(viewdirs) broadcast over samples
//   ZI/models.py:939-951, 1223-1234, 1251   lin_second_stage_i (+skip concat after layer 0), rgb_layer, sigmoid, padding
//
// Design (CDNA4, not a translation of the nn.Linear chain):
//   * the whole chain runs TRANSPOSED, activations^T = W . x^T, on v_mfma_f32_16x16x32_bf16: a result tile (16 output
//     features x 16 samples) has the sample on the lane (col = lane & 15) and rows 4*(lane>>4) + r in its 4 registers, and
//     two such tiles (32 consecutive output features) converted pairwise to bf16 ARE the B operand of the next layer's MFMA
//     for that 32-feature k-block: lane (col, q) element j <-> feature 32*kb + 16*(j>>2) + 4*q + (j&3).  Activations never
//     leave the register file: no LDS round trip, no barrier between the 8+ layers.
//   * weights are the A operand, pre-packed at model-create time into exactly that per-lane order, one 1 KiB fragment per
//     (16 output rows, 32-feature k-block), streamed L2 -> LDS by LDS-DMA through a 3 x 32 KiB ring shared by the 4 waves.
//   * ONE WAVE OWNS 64 SAMPLES (4 column tiles) in the hidden layers: every fragment read from LDS feeds 4 MFMAs.  Round 1
//     ran 32 samples per wave on v_mfma_f32_32x32x16_bf16 (1 MFMA per fragment): profiles/r02_mfma_shape*_microbench.txt
//     put that structure's ceiling at 1.58 PFLOP/s (the chip holds 1.65-1.7 GHz under it) against 1.85 PFLOP/s at 2.13 GHz
//     for 16x16x32 with 4 MFMAs per fragment; per fragment the LDS-DMA issue, the hand-shake and the ds_read are paid once.
//   * the density trunk, the heads and view layers 0/1 (the skip layer, whose three operand sets would need ~400 registers at
//     64 samples) run at HALF WIDTH (2 column tiles = 32 samples) once per half; their weights sit on the tape twice.
//   * the 27 direction-encoding features are computed once per ray by a small pre-kernel and ride through view layers 0 and 1
//     as one extra zero-padded 32-feature k-block, so every GEMM has K % 32 == 0;
//   * nothing but the weight tape is read from global memory after the tile's input loads: all biases sit in LDS and enter
//     as the C operand of each accumulator chain's first MFMA.
//   * NLR_PREC_FAST never forms the bottleneck.  density_layer.2 (64 -> 256) has no activation behind it (models.py:1157-1158:
//     bottleneck = x), so b = W2.h + c2 is linear in the trunk's hidden vector h = relu(W0.f + c0), and the head layer H1, view
//     layer 0 and the skip columns of view layer 1 are linear in b in front of their ReLU.  build_level multiplies W2 into those
//     three once per model (products in double, rounded once); on the tape H1 has K = 64 instead of 256, view layer 0 reads
//     [h | enc] (3 k-blocks instead of 9), view layer 1 [x | h | enc], and D2 is the single 32-row unit that holds row 0, the raw
//     density, with the fragments and the MFMA order it always had: density and everything computed from it keep their bits.
//     Per wave and 256-sample tile at width 256 with both heads: 4 432 MFMAs and 1 368 fragments instead of 6 112 and 2 056.
//     The other two precisions are the exact-parity modes and run the reference's layers as they are.
//   * precision: NLR_PREC_FAST = trunk + heads in split-bf16 (W = Wh + Wl, x = xh + xl, three MFMAs: ~2^-16), view MLP bf16;
//     NLR_PREC_MIXED = trunk + heads on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32); NLR_PREC_F32 = everything exact f32
//     (the whole chain at half width, twice per tile).
#pragma once
#include "nlr_kernels.h"
#include "nlr_tape.h"  // NLR_CHUNK_FRAGS, the tile programs

#include <type_traits>

// ---- weight tape: global -> LDS by LDS-DMA (triple buffered), shared by the 4 waves of a workgroup ----------------
// A chunk is 32 KiB = 32 fragments of 1 KiB (one fragment = the A operand of one MFMA for all 64 lanes).  Every
// wave needs every fragment (each wave owns its samples and all output features), so staging through LDS cuts the
// L2 -> CU weight traffic 4x against per-wave global loads and puts the fragment reads on ds_read_b128.
// The refill is `global_load_lds_dwordx4` (one fragment = one wave-instruction, lane-linear in LDS, which is the
// fragment layout): no VGPR staging and no ds_write pass.
// Schedule inside chunk c (f = fragment position, all positions are compile-time after unrolling):
//   f = NLR_SIG_F   s_waitcnt vmcnt(0) (this wave's quarter of chunk c+1, requested at (NLR_POLL_F, c-1), has landed); signal
//   f = NLR_POLL_F  once all four waves have signalled, each wave requests its quarter (8 fragments) of chunk c+2 into LDS
//                   buffer (c+2)%3 = the buffer of chunk c-1 (hand-shake: see Tape::signal)
//   every f: the fragment f+NLR_PF is requested into a register ring right after fragment f is consumed; near the end of a chunk
//            these requests run into chunk c+1, so no LDS latency is exposed at a chunk boundary.
// GEMMs follow each other on the tape without padding: a GEMM that starts at position F0 of a chunk simply continues the
// position count (all GEMM sizes are compile-time); only the end of a tile's program is padded to a chunk boundary.
#define NLR_CHUNK_SLOTS (NLR_CHUNK_FRAGS * 64)   // uint4 slots per chunk
#define NLR_NBUF 3
#ifndef NLR_SIG_F
#define NLR_SIG_F 8
#endif
#ifndef NLR_POLL_F
#define NLR_POLL_F 22
#endif
#ifndef NLR_PF
#define NLR_PF 8                                 // fragment read-ahead (register ring); must divide NLR_CHUNK_FRAGS
#endif
typedef const __attribute__((address_space(1))) void *nlr_gptr;
typedef __attribute__((address_space(3))) void *nlr_lptr;
struct Tape {
    const uint4 *__restrict__ base;
    uint4 *lds;  // [NLR_NBUF][NLR_CHUNK_SLOTS]
    uint4 ring[NLR_PF];
    // cur: chunks consumed so far by this workgroup (runs on across tiles); nxt: tape index of the next chunk to request
    // (wraps at `total`, the chunks one tile consumes: a persistent workgroup streams the tape round and round);
    // b0/b1/b2: LDS buffer (0..2) of chunks cur, cur+1, cur+2
    int cur, nxt, total, tid, lane;
    int b0, b1, b2;
    __device__ __forceinline__ uint4 *buf(int b) const { return lds + b * NLR_CHUNK_SLOTS; }
    // this wave's quarter of chunk c: fragments 8w .. 8w+7, one LDS-DMA instruction each (LDS address = M0 + 16*lane).
    // Inline asm on purpose: behind the builtin hipcc puts an s_waitcnt vmcnt(0) in front of the next ds_read (it cannot
    // tell the DMA's LDS target from the ring reads), which would expose the whole L2 latency once per chunk.  An asm
    // DMA is invisible to hipcc's counters; `signal()` holds the one wait that retires it.  M0 is saved and restored.
    __device__ __forceinline__ void dma(int b) {  // tape chunk `nxt` -> LDS buffer b
        const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6);
        const uint64_t g = reinterpret_cast<uint64_t>(base) + (uint64_t)(uint32_t)nxt * (NLR_CHUNK_SLOTS * 16) + w * 8192u;
        const uint32_t l = (uint32_t)(uintptr_t)(nlr_lptr)buf(b) + w * 8192u;
        nxt = (nxt + 1 == total) ? 0 : nxt + 1;
        const uint32_t v = (uint32_t)lane * 16u;
        uint32_t keep;
        // The instruction offset advances the global AND the LDS address (LDS address = M0 + offset + 16 * lane), so four
        // pieces share one M0 value and one SGPR base.
        asm volatile(
            "s_mov_b32 %[k], m0\n\t"
            "s_mov_b32 m0, %[l]\n\ts_nop 0\n\t"
            "global_load_lds_dwordx4 %[v], %[g0]\n\t"
            "global_load_lds_dwordx4 %[v], %[g0] offset:1024\n\t"
            "global_load_lds_dwordx4 %[v], %[g0] offset:2048\n\t"
            "global_load_lds_dwordx4 %[v], %[g0] offset:3072\n\t"
            "s_add_u32 m0, %[l], 0x1000\n\ts_nop 0\n\t"
            "global_load_lds_dwordx4 %[v], %[g4]\n\t"
            "global_load_lds_dwordx4 %[v], %[g4] offset:1024\n\t"
            "global_load_lds_dwordx4 %[v], %[g4] offset:2048\n\t"
            "global_load_lds_dwordx4 %[v], %[g4] offset:3072\n\t"
            "s_mov_b32 m0, %[k]"
            : [k] "=&s"(keep)
            : [v] "v"(v), [l] "s"(l), [g0] "s"(g), [g4] "s"(g + 4096)
            : "memory", "scc");
    }
    // Workgroup hand-shake without s_barrier (a barrier per chunk charges every wave the slowest wave's drift each time):
    //   (NLR_SIG_F, c)    own quarter of chunk c+1 has landed (vmcnt) and the last fragment of chunk c-1 is consumed
    //                     -> lane 0 adds 1 to an LDS counter
    //   (NLR_POLL_F-2, c) the counter is read; (NLR_POLL_F, c) spin until it shows 4 (c+1): every wave is past its signal of
    //                     chunk c, so chunk c+1 is complete and the buffer of chunk c-1 is free -> DMA c+2
    // LDS accesses of one CU are served in order by one unit, so counter and data need no fence beyond the vmcnt wait in
    // front of the signal.  All three steps are single asm statements: C++ control flow here would split the unrolled
    // MFMA chain into basic blocks and lose the ds_read / MFMA interleave.
    uint32_t *sig;
    uint32_t sig_addr, seen;
    __device__ __forceinline__ void signal() {
        uint64_t sv;
        asm volatile(
            "s_waitcnt vmcnt(0)\n\t"
            "s_mov_b64 %[sv], exec\n\t"
            "s_mov_b64 exec, 1\n\t"
            "ds_add_u32 %[a], %[one]\n\t"
            "s_mov_b64 exec, %[sv]"
            : [sv] "=&s"(sv)
            : [a] "v"(sig_addr), [one] "v"(1u)
            : "memory");
    }
    __device__ __forceinline__ void peek() { seen = *reinterpret_cast<volatile __attribute__((address_space(3))) uint32_t *>(sig_addr); }
    __device__ __forceinline__ void await() {
        const uint32_t target = 4u * (uint32_t)(cur + 1);
        uint32_t t;
        asm volatile(
            "1:\n\t"
            "v_readfirstlane_b32 %[t], %[seen]\n\t"
            "s_cmp_ge_u32 %[t], %[target]\n\t"
            "s_cbranch_scc1 2f\n\t"
            "s_sleep 1\n\t"
            "ds_read_b32 %[seen], %[a]\n\t"
            "s_waitcnt lgkmcnt(0)\n\t"
            "s_branch 1b\n"
            "2:"
            : [seen] "+v"(seen), [t] "=&s"(t)
            : [a] "v"(sig_addr), [target] "s"(target)
            : "memory", "scc");
    }
    __device__ __forceinline__ void prologue() {
        cur = 0;
        nxt = 0;
        b0 = 0, b1 = 1, b2 = 2;
        if (tid == 0) *sig = 0u;
        dma(0);
        dma(1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();  // both chunks and the bias block are visible to every wave
#pragma unroll
        for (int f = 0; f < NLR_PF; ++f) ring[f] = buf(0)[f * 64 + lane];
    }
    // bookkeeping at fragment position F of the current chunk; returns the fragment (raw 16 bytes per lane).
    // IGNORED: a padding step - the fragment at F is not used, and neither is any fragment before the next chunk boundary, so
    // the read-ahead only has to resume where it reaches into the next chunk
    template <int F, bool IGNORED = false>
    __device__ __forceinline__ uint4 step() {
        static_assert(F >= 0 && F < NLR_CHUNK_FRAGS, "tape position");
        if constexpr (F == NLR_SIG_F) signal();
        if constexpr (F == NLR_POLL_F - 2) peek();
        if constexpr (F == NLR_POLL_F) {
            await();
            dma(b2);
        }
        const uint4 a = ring[F % NLR_PF];
        if constexpr (F + NLR_PF < NLR_CHUNK_FRAGS) {
            if constexpr (!IGNORED) ring[F % NLR_PF] = buf(b0)[(F + NLR_PF) * 64 + lane];
        } else {
            ring[F % NLR_PF] = buf(b1)[(F + NLR_PF - NLR_CHUNK_FRAGS) * 64 + lane];
        }
        if constexpr (F == NLR_CHUNK_FRAGS - 1) {
            ++cur;
            const int t = b0;
            b0 = b1, b1 = b2, b2 = t;
        }
        return a;
    }
};

template <typename T>
__device__ __forceinline__ T nlr_as(const uint4 &v) {
    return __builtin_bit_cast(T, v);
}

template <int I>
using ic = std::integral_constant<int, I>;

// steps from position F to the next chunk boundary (bookkeeping positions must still run; the fragments are ignored)
template <int F>
__device__ __forceinline__ void nlr_pad(Tape &tp) {
    if constexpr (F % NLR_CHUNK_FRAGS != 0) {
        (void)tp.template step<F % NLR_CHUNK_FRAGS, true>();
        __builtin_amdgcn_sched_barrier(0);
        nlr_pad<F % NLR_CHUNK_FRAGS + 1>(tp);
    }
}

// K steps from position F whose fragments are ignored (a part of the tile's program that this launch does not run): whole
// chunks in a runtime loop, the remainder unrolled
template <int F, int K>
__device__ __forceinline__ void nlr_skip_few(Tape &tp) {
    if constexpr (K > 0) {
        (void)tp.template step<F % NLR_CHUNK_FRAGS>();
        __builtin_amdgcn_sched_barrier(0);
        nlr_skip_few<F % NLR_CHUNK_FRAGS + 1, K - 1>(tp);
    }
}
template <int F, int K>
__device__ __forceinline__ void nlr_skip(Tape &tp) {
    for (int c = 0; c < K / NLR_CHUNK_FRAGS; ++c) nlr_skip_few<F, NLR_CHUNK_FRAGS>(tp);
    nlr_skip_few<F, K % NLR_CHUNK_FRAGS>(tp);
}

// ---- register tiles ---------------------------------------------------------------------------------------------------
// N = 16-sample column tiles held by the wave (4 = 64 samples, 2 = 32 samples: half width).
// Unit: 32 output rows x 16N samples of f32 accumulators: a[jb][n][r] on lane (col, rb) is row 16*jb + 4*rb + r of column
//       tile n, sample 16*n + col.
// BT:   32 input features x 16N samples as MFMA B operands: n[t] element j on lane (col, q) is feature 16*(j>>2) + 4*q + (j&3).
//       pack(Unit) -> BT is lane-local: BT.n[t][4*jb + r] = bf16(Unit.a[jb][t][r]).
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int N>
struct BT {
    bf16x8 n[N];
};
template <int N>
struct Unit {
    f32x4 a[2][N];
};

// epilogue piece P of 4N: column tile P >> 2, row block (P >> 1) & 1, register pair P & 1 -> one packed dword
// ReLU is applied AFTER the conversion, on the packed pair: a negative bf16 is a negative int16, so one v_pk_max_i16
// against zero clears two values (-0.0 -> +0.0).
// OFF: the half-width GEMMs (N = 2) address column tiles OFF .. OFF+N-1 of a full-width BT<ND>
template <bool RELU, int P, int OFF, int N, int ND>
__device__ __forceinline__ void nlr_pack_piece(BT<ND> &dst, const Unit<N> &src) {
    constexpr int n = P >> 2, jb = (P >> 1) & 1, pr = P & 1;
    const f32x2 x = {src.a[jb][n][2 * pr], src.a[jb][n][2 * pr + 1]};
    bf16x2 v = __builtin_convertvector(x, bf16x2);  // one v_cvt_pk_bf16_f32 (RNE)
    if (RELU) {
        const s16x2 z = {0, 0};
        v = __builtin_bit_cast(bf16x2, __builtin_elementwise_max(__builtin_bit_cast(s16x2, v), z));
    }
    dst.n[OFF + n][4 * jb + 2 * pr] = v[0];
    dst.n[OFF + n][4 * jb + 2 * pr + 1] = v[1];
}
// hi = bf16(x), lo = bf16(x - hi)   (x - hi is exact in f32)
template <bool RELU, int P, int OFF, int N, int ND>
__device__ __forceinline__ void nlr_split_piece(BT<ND> &hi, BT<ND> &lo, const Unit<N> &src) {
    constexpr int n = P >> 2, jb = (P >> 1) & 1, pr = P & 1;
    f32x2 x = {src.a[jb][n][2 * pr], src.a[jb][n][2 * pr + 1]};
    if (RELU) x = __builtin_elementwise_max(x, (f32x2){0.0f, 0.0f});
    const bf16x2 h = __builtin_convertvector(x, bf16x2);
    const bf16x2 l = __builtin_convertvector(x - __builtin_convertvector(h, f32x2), bf16x2);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        hi.n[OFF + n][4 * jb + 2 * pr + e] = h[e];
        lo.n[OFF + n][4 * jb + 2 * pr + e] = l[e];
    }
}
template <bool RELU, int OFF, int N, int ND, int P = 0>
__device__ __forceinline__ void nlr_pack_all(BT<ND> &dst, const Unit<N> &src) {
    if constexpr (P < 4 * N) {
        nlr_pack_piece<RELU, P, OFF>(dst, src);
        nlr_pack_all<RELU, OFF, N, ND, P + 1>(dst, src);
    }
}
template <bool RELU, int OFF, int N, int ND, int P = 0>
__device__ __forceinline__ void nlr_split_all(BT<ND> &hi, BT<ND> &lo, const Unit<N> &src) {
    if constexpr (P < 4 * N) {
        nlr_split_piece<RELU, P, OFF>(hi, lo, src);
        nlr_split_all<RELU, OFF, N, ND, P + 1>(hi, lo, src);
    }
}
template <bool RELU, int N>
__device__ __forceinline__ void nlr_act_unit(Unit<N> &u) {
    if (RELU) {
#pragma unroll
        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
            for (int n = 0; n < N; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) u.a[jb][n][r] = fmaxf(u.a[jb][n][r], 0.0f);
    }
}

// ---- MFMA steps: one tape fragment (16 output rows) against every column tile of the wave ---------------------------------
// FIRST: the accumulator chain starts here, C = the bias rows of this row block
template <bool FIRST, int OFF, int N, int ND>
__device__ __forceinline__ void nlr_mma_bf16(f32x4 (&acc)[N], const f32x4 &bias, const uint4 &a, const BT<ND> &b) {
#pragma unroll
    for (int n = 0; n < N; ++n)
        acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(nlr_as<bf16x8>(a), b.n[OFF + n], FIRST ? bias : acc[n], 0, 0, 0);
}
// Split-bf16 ("bf16x3"): W = Wh + Wl, x = xh + xl (each part bf16), W.x ~= Wh.xh + Wh.xl + Wl.xh with f32
// accumulation: 16 mantissa bits per operand (relative error ~2^-16) at 3/16 of the exact-f32 MFMA cost.
template <bool FIRST, int OFF, int N, int ND>
__device__ __forceinline__ void nlr_mma_x3(f32x4 (&acc)[N], const f32x4 &bias, const uint4 &ah, const uint4 &al, const BT<ND> &bh,
                                           const BT<ND> &bl) {
#pragma unroll
    for (int n = 0; n < N; ++n) {
        acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(nlr_as<bf16x8>(ah), bh.n[OFF + n], FIRST ? bias : acc[n], 0, 0, 0);
        acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(nlr_as<bf16x8>(ah), bl.n[OFF + n], acc[n], 0, 0, 0);
        acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(nlr_as<bf16x8>(al), bh.n[OFF + n], acc[n], 0, 0, 0);
    }
}
// exact-f32 MFMA (v_mfma_f32_16x16x4_f32): one fragment (float4 per lane) carries the 4 k-steps of one 16-feature input row
// block: element e of lane (m, q) is W[row m][16*J + 4*q + e], and register e of the input accumulator tile is exactly that
// feature on lane (col, q).
template <bool FIRST, int N>
__device__ __forceinline__ void nlr_mma_f32(f32x4 (&acc)[N], const f32x4 &bias, const uint4 &a, const f32x4 (&in)[N]) {
    const f32x4 af = nlr_as<f32x4>(a);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int n = 0; n < N; ++n)
            acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[e], in[n][e], (FIRST && e == 0) ? bias : acc[n], 0, 0, 0);
}

// sum / max over the 4 lanes (col, q = 0..3) that hold the rows of one sample: v_permlane16_swap exchanges the odd 16-lane
// rows of its first operand with the even rows of its second (given one value twice it returns [row0,row0,row2,row2] and
// [row1,row1,row3,row3]), v_permlane32_swap does the same with 32-lane halves: two VALU exchanges, no LDS traffic.
__device__ __forceinline__ float nlr_q_sum(float v) {
    uint32_t u = __builtin_bit_cast(uint32_t, v);
    auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    v = __builtin_bit_cast(float, (uint32_t)a[0]) + __builtin_bit_cast(float, (uint32_t)a[1]);
    u = __builtin_bit_cast(uint32_t, v);
    auto b = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __builtin_bit_cast(float, (uint32_t)b[0]) + __builtin_bit_cast(float, (uint32_t)b[1]);
}
__device__ __forceinline__ float nlr_q_max(float v) {
    uint32_t u = __builtin_bit_cast(uint32_t, v);
    auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    v = fmaxf(__builtin_bit_cast(float, (uint32_t)a[0]), __builtin_bit_cast(float, (uint32_t)a[1]));
    u = __builtin_bit_cast(uint32_t, v);
    auto b = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return fmaxf(__builtin_bit_cast(float, (uint32_t)b[0]), __builtin_bit_cast(float, (uint32_t)b[1]));
}

// DPP moves inside a 16-lane row (= the 16 samples of one column tile); lanes without a source lane read 0
template <int CTRL>
__device__ __forceinline__ float nlr_dpp0(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float nlr_row_incl_scan(float v) {  // Hillis-Steele over the 16 lanes of a row (row_shr:1,2,4,8)
    v += nlr_dpp0<0x111>(v);
    v += nlr_dpp0<0x112>(v);
    v += nlr_dpp0<0x114>(v);
    v += nlr_dpp0<0x118>(v);
    return v;
}
__device__ __forceinline__ float nlr_row_shr1(float v) { return nlr_dpp0<0x111>(v); }  // lane c <- lane c-1, lane 0 <- 0
__device__ __forceinline__ float nlr_row_sum(float v) {  // butterfly: every lane of the row gets the row's sum
    v += nlr_dpp0<0xB1>(v);   // quad_perm [1,0,3,2]
    v += nlr_dpp0<0x4E>(v);   // quad_perm [2,3,0,1]
    v += nlr_dpp0<0x141>(v);  // row_half_mirror
    v += nlr_dpp0<0x140>(v);  // row_mirror
    return v;
}

// ---- GEMM driver ---------------------------------------------------------------------------------------------------------
// One GEMM = OT output units (32 rows; RH = 2 row blocks of 16, or RH = 1: only the first 16 rows exist) x KG k-groups
// (32 input features per group on the bf16 paths, 16 on the exact-f32 path), N column tiles.  Tape order: unit-major, then
// k-group, then row block: step (o, g, j) consumes FPS fragments (2 = the hi / lo pair of the split-bf16 path) and issues
// N (3N, 4N) MFMAs.  One accumulator unit runs all its steps; the finished unit's epilogue (bf16 pack + ReLU, or hi/lo split)
// is cut into NP pieces issued behind the next unit's MFMAs, the next unit's bias rows are read from LDS a few steps early,
// and the issue order is pinned with sched_barrier(0) per step (left alone, hipcc sinks the ring's ds_reads next to their
// use and every MFMA waits out the LDS latency).
//   F0     tape position (fragments since a chunk boundary) at which this GEMM starts
//   NPP    > 0: `pend(ic<p>)`, p < NPP, are the epilogue pieces of the PREVIOUS GEMM's last unit; they run behind the MFMAs of
//          this GEMM's first steps and are complete before step PBY (the first step that reads that unit)
//   DEFER  the last unit of this GEMM is handed back raw in `last` (its epilogue becomes the next GEMM's `pend`) instead of
//          being post-processed serially behind the last MFMA, where nothing would hide it
//   bias(ic<o>, f32x4 (&b)[2]);  mma(unit&, ic<g>, ic<j>, f0, f1, biasrow);  epi(ic<o>, ic<p>, unit);  pend(ic<p>);  bg(ic<step>)
constexpr int nlr_ceil_div(int a, int b) { return (a + b - 1) / b; }

template <int O, int P0, int P1, class Epi, int N>
__device__ __forceinline__ void nlr_pieces(const Epi &epi, const Unit<N> &u) {
    if constexpr (P0 < P1) {
        epi(ic<O>{}, ic<P0>{}, u);
        nlr_pieces<O, P0 + 1, P1>(epi, u);
    }
}
template <int P0, int P1, class Pend>
__device__ __forceinline__ void nlr_pend(const Pend &pend) {
    if constexpr (P0 < P1) {
        pend(ic<P0>{});
        nlr_pend<P0 + 1, P1>(pend);
    }
}

template <int OT, int KG, int RH, int N, int FPS, int F0, int NP, int NPP, int PBY, bool DEFER, int IDX, class Bias, class Mma, class Epi,
          class Pend, class Bg>
__device__ __forceinline__ void nlr_run(Tape &tp, Unit<N> &prev, Unit<N> &cur, f32x4 (&bcur)[2], f32x4 (&bnxt)[2], Unit<N> &last,
                                        const Bias &bias, const Mma &mma, const Epi &epi, const Pend &pend, const Bg &bg) {
    constexpr int SPU = KG * RH;                      // steps per unit
    constexpr int D = SPU > 1 ? 1 : 0;                // the previous unit's last MFMAs retire during step 0
    constexpr int PPS = nlr_ceil_div(NP, SPU - D);    // epilogue pieces per step
    constexpr int IG = SPU >= 4 ? SPU - 3 : SPU - 1;  // step at which the next unit's bias rows are requested
    if constexpr (IDX < OT * SPU) {
        constexpr int o = IDX / SPU, s = IDX % SPU, g = s / RH, j = s % RH;
        if constexpr (s == 0) {
            if constexpr (o > 0) {
                prev = cur;
                bcur[0] = bnxt[0];
                bcur[1] = bnxt[1];
            } else {
                bias(ic<0>{}, bcur);
            }
        }
        constexpr int P0 = (F0 + IDX * FPS) % NLR_CHUNK_FRAGS;
        const uint4 f0 = tp.template step<P0>();
        uint4 f1 = f0;
        if constexpr (FPS == 2) f1 = tp.template step<(P0 + 1) % NLR_CHUNK_FRAGS>();
        mma(cur, ic<g>{}, ic<j>{}, f0, f1, bcur[j]);
        if constexpr (o > 0) {
            if constexpr (s >= D && (s - D) * PPS < NP)
                nlr_pieces<o - 1, (s - D) * PPS, ((s - D + 1) * PPS < NP ? (s - D + 1) * PPS : NP)>(epi, prev);
        } else if constexpr (NPP > 0) {
            constexpr int PP = nlr_ceil_div(NPP, PBY - D);
            if constexpr (s >= D && (s - D) * PP < NPP) nlr_pend<(s - D) * PP, ((s - D + 1) * PP < NPP ? (s - D + 1) * PP : NPP)>(pend);
        }
        if constexpr (s == IG && o + 1 < OT) bias(ic<o + 1>{}, bnxt);
        bg(ic<IDX>{});
        __builtin_amdgcn_sched_barrier(0);
        nlr_run<OT, KG, RH, N, FPS, F0, NP, NPP, PBY, DEFER, IDX + 1>(tp, prev, cur, bcur, bnxt, last, bias, mma, epi, pend, bg);
    } else {
        if constexpr (DEFER) last = cur;
        else nlr_pieces<OT - 1, 0, NP>(epi, cur);
    }
}
// plain form: no pending pieces, no background work, serial epilogue of the last unit
template <int OT, int KG, int RH, int N, int FPS, int F0, int NP, class Bias, class Mma, class Epi>
__device__ __forceinline__ void nlr_gemm(Tape &tp, const Bias &bias, const Mma &mma, const Epi &epi) {
    Unit<N> prev, cur, last;
    f32x4 bc[2], bn[2];
    nlr_run<OT, KG, RH, N, FPS, F0, NP, 0, 1, false, 0>(tp, prev, cur, bc, bn, last, bias, mma, epi, [](auto) {}, [](auto) {});
}
// software-pipelined across GEMMs: pend = the previous GEMM's deferred unit, last = this GEMM's (when DEFER)
// bg(ic<step>): background work of the caller (compositing pieces), one call per step
template <int OT, int KG, int RH, int N, int F0, int NP, int NPP, int PBY, bool DEFER, class Bias, class Mma, class Epi, class Pend, class Bg>
__device__ __forceinline__ void nlr_gemm_pipe(Tape &tp, Unit<N> &last, const Bias &bias, const Mma &mma, const Epi &epi, const Pend &pend,
                                              const Bg &bg) {
    Unit<N> prev, cur;
    f32x4 bc[2], bn[2];
    nlr_run<OT, KG, RH, N, 1, F0, NP, NPP, PBY, DEFER, 0>(tp, prev, cur, bc, bn, last, bias, mma, epi, pend, bg);
}
template <int OT, int KG, int RH, int N, int F0, int NP, int NPP, int PBY, bool DEFER, class Bias, class Mma, class Epi, class Pend>
__device__ __forceinline__ void nlr_gemm_pipe(Tape &tp, Unit<N> &last, const Bias &bias, const Mma &mma, const Epi &epi, const Pend &pend) {
    nlr_gemm_pipe<OT, KG, RH, N, F0, NP, NPP, PBY, DEFER>(tp, last, bias, mma, epi, pend, [](auto) {});
}

// Diagnostic builds only (-DNLR_STAMPS, scripts/diag_build.sh): s_memtime at the phase boundaries of every workgroup's LAST tile,
// written to a buffer of their own (nlr_stamp_buf) that nothing else reads; the product build contains no stamp.
#ifdef NLR_STAMPS
#define NLR_NSTAMP 24
extern __device__ unsigned long long nlr_stamp_buf[1024 * NLR_NSTAMP];  // defined in nlr_mlp_inst.hip (same translation unit)
#define NLR_STAMP(i)                                          \
    do {                                                      \
        __builtin_amdgcn_sched_barrier(0);                    \
        stamps[i] = __builtin_amdgcn_s_memtime();             \
        __builtin_amdgcn_sched_barrier(0);                    \
    } while (0)
#else
#define NLR_STAMP(i) do { } while (0)
#endif

// WT = view width / 32, BW = bottleneck / 32, FT = ceil(F / 32) grid-feature k-blocks, HT = head hidden units of 32 (0, 2 or 4)
// PREC: NLR_PREC_F32 (all f32), NLR_PREC_MIXED (trunk+heads f32, view bf16), NLR_PREC_FAST (trunk+heads bf16x3, view bf16)
#define NLR_BIAS_MAX 3072  // floats of LDS reserved for the bias block (12 KiB)
#define NLR_TILE 256       // samples per workgroup tile: 4 waves x 64
// Input staging (per wave): the NEXT tile's grid features (piece-major: one 1 KiB LDS-DMA per 4-feature piece and wave), the
// direction-encoding rows of its rays (one gathering LDS-DMA) [and its sample distances] land in LDS while the current tile
// computes; a tile starts by reading its inputs from LDS.  No registers and ~1 issue slot per KiB for the prefetch.
#define NLR_STAGE_PIECES 11                           // up to 44 grid features are staged (more: direct global loads)
#define NLR_STAGE_ENC (NLR_STAGE_PIECES * 256)        // float offset of the enc rows [n-tile][row block][q] x 4 floats
#define NLR_STAGE_TD (NLR_STAGE_ENC + 128)            // float offset of t_k [64], t_k+1 [64], |d| [64], last-sample flag [64]
#define NLR_STAGE_FLOATS (NLR_STAGE_TD + 256)
// COMP: compositing mode (render path).  A 32-sample half of a wave is one segment of one ray (S % 32 == 0): the kernel turns the
//   density into segment-local alpha weights w'_k = alpha_k exp(-sum_{j<k, j in segment} sigma_j delta_j) (16-lane DPP scan) and
//   writes, instead of 24 floats per SAMPLE (class probabilities, intensity, rgb), one 32-float record per SEGMENT:
//   [0,K) sum w' p_c, [K] sum w' intensity, [29,32) sum w' rgb.  nlr_composite_kernel scales each record by the transmittance at
//   its segment start.  All of it is VALU work issued piece by piece behind the MFMAs of view layers 0 and 1.
// CM: 0 = per-sample outputs, 1 = COMP, 2 = LiDAR-only compositing (LIDAR): trunk + heads + segment records and NO view MLP, for
//   renders whose caller wants no rgb (nlr_render_lidar).  The tile's program is [T | T] on a tape of its own (MlpParams.tape is the
//   level's LiDAR tape: the view layers' fragments never enter LDS), the direction encoding is neither staged nor read, and slots
//   [29,32) of every record hold 0.  Trunk, heads and the 35 compositing pieces are the code of mode 1, so density and records
//   [0,K] are the same bits.  The pieces run serially behind each half's heads (there is no view layer 0 to hide them); the next
//   tile's inputs are requested once both halves have read theirs and land under the second half's trunk.  WT does not enter.
template <int WT, int BW, int FT, int HT, int PREC, int CM>
__global__ void __launch_bounds__(256, 1) nlr_mlp_kernel(MlpParams P) {
    constexpr bool COMP = CM != 0, LIDAR = CM == 2;
    static_assert(!LIDAR || PREC == NLR_PREC_FAST, "the LiDAR-only instances exist for NLR_PREC_FAST");
    __shared__ __align__(16) uint4 lds_tape[NLR_NBUF * NLR_CHUNK_SLOTS];
    __shared__ __align__(16) float lds_bias[NLR_BIAS_MAX];
    __shared__ __align__(16) float lds_stage[4 * NLR_STAGE_FLOATS];
    __shared__ uint32_t lds_sig;
    constexpr bool VIEW_F32 = (PREC == NLR_PREC_F32);
    constexpr bool X3 = (PREC == NLR_PREC_FAST);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, q = lane >> 4;
    constexpr int HTA = HT > 0 ? HT : 1;
    // FOLD (NLR_PREC_FAST): density_layer.2 has no activation behind it, so the bottleneck b = W2.h + c2 is linear in the trunk's hidden
    // vector h = relu(W0.f + c0), and every consumer of b is linear in b in front of its own ReLU.  build_level multiplies W2 into the
    // head layer H1, view layer 0 and the skip columns of view layer 1 once per model; the kernel never forms the bottleneck: those
    // three GEMMs read the PG.KB = 2 k-blocks of h, and D2 keeps the one output unit (PG.D2U = 1) that holds row 0, the raw density (same
    // fragments, same MFMA order as the unfolded unit 0: density and everything derived from it keep their bits).
    // PG: the tile's program on the tape and the offsets of the bias block (nlr_tape.h; the host checks what it built against the same table)
    constexpr MlpProgram PG = nlr_mlp_program(WT, BW, FT, HT, PREC, CM);
    // (named as plain constants: used through PG inside the GEMM lambdas, 14 instances came out with another register allocation)
    constexpr int KB = PG.KB, FR_D0 = PG.FR_D0, FR_D2 = PG.FR_D2, FR_H1 = PG.FR_H1, FR_T = PG.FR_T, FR_V0 = PG.FR_V0, FR_V1 = PG.FR_V1;
    constexpr int FR_HALF = PG.FR_HALF, F_HID = PG.F_HID, F_END = PG.F_END;
    constexpr int OB_D0 = PG.OB_D0, OB_D2 = PG.OB_D2, OB_H1 = PG.OB_H1, OB_H2 = PG.OB_H2, OB_V0 = PG.OB_V0, OB_V1 = PG.OB_V1, OB_VL = PG.OB_VL;
    static_assert(PG.FR_HL % NLR_CHUNK_FRAGS == 0, "hidden view layers must cover whole chunks (width 128 or 256)");
    // The next tile's inputs are requested by LDS-DMA at tape position STAGE_AT of the tile's program and read at the start of the next
    // tile with no wait of their own: a signal() of the tape (position NLR_SIG_F of every chunk, s_waitcnt vmcnt(0): it retires every
    // load of the wave) has to lie between the request and the end of the program, padding steps included.  SIG_AT is the first one.
    // The hidden view layers are whole chunks, so with at least one of them the condition holds; without one (view depth 2) and for
    // the LiDAR-only program it depends on where the request falls in its chunk, and a tile that has no such signal waits itself.
    constexpr int STAGE_AT = LIDAR ? FR_T : F_HID, PROG_END = nlr_ceil_div(PG.frags(2), NLR_CHUNK_FRAGS) * NLR_CHUNK_FRAGS;
    constexpr int SIG_AT = STAGE_AT <= NLR_SIG_F ? NLR_SIG_F : nlr_ceil_div(STAGE_AT - NLR_SIG_F, NLR_CHUNK_FRAGS) * NLR_CHUNK_FRAGS + NLR_SIG_F;
    constexpr bool STAGE_SIG = SIG_AT < PROG_END;         // (without hidden layers)
    static_assert(!LIDAR || STAGE_SIG, "LiDAR-only: no tape signal between the request of the next tile's inputs and their first read");

    const uint32_t ntiles = (P.M + NLR_TILE - 1) / NLR_TILE;
    for (uint32_t i = threadIdx.x * 4; i < P.bias_count; i += 1024)
        *reinterpret_cast<f32x4 *>(lds_bias + i) = *reinterpret_cast<const f32x4 *>(P.bias_all + i);

    Tape tp;
    tp.base = P.tape;
    tp.lds = lds_tape;
    tp.sig = &lds_sig;
    tp.sig_addr = (uint32_t)(uintptr_t)(nlr_lptr)&lds_sig;
    // without the view MLP (density / semantic / intensity only: not a hot path) the view layers' fragments are stepped over
    tp.total = (LIDAR || P.rgb) ? (int)P.tape_chunks : nlr_ceil_div(VIEW_F32 ? FR_T : F_HID, NLR_CHUNK_FRAGS);
    tp.tid = threadIdx.x;
    tp.lane = lane;
    tp.prologue();  // ends with __syncthreads(): the bias block is visible too

    auto nop = [](auto) {};
    auto bias_rows = [&](const float *b, f32x4 (&out)[2]) {  // rows 4q..4q+3 of both 16-row blocks of a unit
        out[0] = *reinterpret_cast<const f32x4 *>(b + 4 * q);
        out[1] = *reinterpret_cast<const f32x4 *>(b + 16 + 4 * q);
    };

    // ---- input staging (see NLR_STAGE_*).  The wave's 64 samples start at stage_base(tile): `base`, pulled back inside the
    // buffer for the last, partial tile (the samples past M are computed and dropped).
    // (COMP: required, checked by the host.  The feature buffer is followed by >= 1 KiB of workspace: a window that starts inside
    // it may run past its end when M < 64; those samples are computed and dropped.)
    const bool staged = P.feat_piece_major && P.F <= 4 * NLR_STAGE_PIECES && (LIDAR || P.rgb != nullptr);
    float *stg = lds_stage + wave * NLR_STAGE_FLOATS;
    const uint32_t stg_lds = (uint32_t)(uintptr_t)(nlr_lptr)lds_stage + __builtin_amdgcn_readfirstlane(wave) * (NLR_STAGE_FLOATS * 4u);  // uniform
    auto stage_base = [&](uint32_t t) {
        const uint32_t b = t * NLR_TILE + wave * 64;
        return b + 64 <= P.M ? b : (P.M >= 64 ? P.M - 64 : 0);
    };
    auto stage_issue = [&](uint32_t t) {
        const uint32_t b = __builtin_amdgcn_readfirstlane(stage_base(t));
        const uint32_t l0 = stg_lds;
        const uint32_t voff = (uint32_t)lane * 16u;
        uint32_t keep;  // every statement saves and restores M0 itself: nothing is assumed about the code between them
        const uint32_t np = P.F / 4;
        for (uint32_t p = 0; p < np; ++p) {  // one piece = 64 samples x 16 B, contiguous in the piece-major feature buffer
            const uint64_t g = reinterpret_cast<uint64_t>(P.feat) + ((uint64_t)p * P.M + b) * 16u;
            asm volatile("s_mov_b32 %[k], m0\n\ts_mov_b32 m0, %[l]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %[v], %[g]\n\ts_mov_b32 m0, %[k]"
                         : [k] "=&s"(keep)
                         : [v] "v"(voff), [l] "s"(l0 + p * 1024u), [g] "s"(g)
                         : "memory");
        }
        if constexpr (!LIDAR) {  // direction-encoding rows: lane i < 32 fetches the 16 bytes [n-tile i>>3][row block (i>>2)&1][q = i&3]
            // (rows go by the tile's real sample numbers, not by the pulled-back feature window)
            const uint32_t s0 = t * NLR_TILE + wave * 64 + 16u * ((uint32_t)lane >> 3 & 3u);
            const uint32_t ray = (s0 < P.M ? s0 : P.M - 1) / P.S;
            const uint64_t g = reinterpret_cast<uint64_t>(P.enc) + ((uint64_t)ray * 32u + 16u * ((lane >> 2) & 1) + 4u * (lane & 3)) * 4u;
            uint64_t sv;
            asm volatile(
                "s_mov_b64 %[sv], exec\n\t"
                "s_mov_b64 exec, %[lo32]\n\t"
                "s_mov_b32 %[k], m0\n\t"
                "s_mov_b32 m0, %[l]\n\ts_nop 0\n\t"
                "global_load_lds_dwordx4 %[g], off\n\t"
                "s_mov_b32 m0, %[k]\n\t"
                "s_mov_b64 exec, %[sv]"
                : [sv] "=&s"(sv), [k] "=&s"(keep)
                : [g] "v"(g), [l] "s"(l0 + NLR_STAGE_ENC * 4u), [lo32] "s"((uint64_t)0xffffffffull)
                : "memory");
        }
        if constexpr (COMP) {  // per sample (lane i = sample i of the wave): t_k, t_k+1, |d| of its ray, "last sample of an opaque ray"
            const uint32_t sm = t * NLR_TILE + wave * 64 + lane;
            const uint32_t sc = sm < P.M ? sm : P.M - 1;
            const uint32_t ray = sc / P.S, k = sc - ray * P.S;
            const uint64_t g0 = reinterpret_cast<uint64_t>(P.tdist) + ((uint64_t)ray * (P.S + 1) + k) * 4u;
            const uint64_t g2 = reinterpret_cast<uint64_t>(P.dnorm) + (uint64_t)ray * 4u;
            asm volatile(
                "s_mov_b32 %[k], m0\n\t"
                "s_mov_b32 m0, %[l]\n\ts_nop 0\n\t"
                "global_load_lds_dword %[g0], off\n\t"
                "s_add_u32 m0, %[l], 0xfc\n\ts_nop 0\n\t"  // the instruction offset advances the LDS address too: 0xfc + 4 = 0x100
                "global_load_lds_dword %[g0], off offset:4\n\t"
                "s_add_u32 m0, %[l], 0x200\n\ts_nop 0\n\t"
                "global_load_lds_dword %[g2], off\n\t"
                "s_mov_b32 m0, %[k]"
                : [k] "=&s"(keep)
                : [g0] "v"(g0), [g2] "v"(g2), [l] "s"(l0 + NLR_STAGE_TD * 4u)
                : "memory", "scc");
            stg[NLR_STAGE_TD + 192 + lane] = (P.opaque && k == P.S - 1) ? 1.0f : 0.0f;
        }
    };
    if (staged && blockIdx.x < ntiles) {
        stage_issue(blockIdx.x);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }

#ifdef NLR_STAMPS
    unsigned long long stamps[NLR_NSTAMP];
#pragma unroll
    for (int i = 0; i < NLR_NSTAMP; ++i) stamps[i] = 0;
#endif
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t base = tile * NLR_TILE + wave * 64;
    NLR_STAMP(0);
#ifdef NLR_STAMPS
    const unsigned long long rt0 = __builtin_amdgcn_s_memrealtime();
#endif
    // ---- inputs of one 32-sample half: grid features as f32 units (row block J = 2t + jb holds features 16J + 4q + r) and the
    // direction encoding of the sample's ray as one more 32-feature unit; read from the LDS staging area right before the half's
    // trunk (or, outside the staged path, straight from global memory)
    auto load_inputs = [&](auto hh, Unit<2> (&fin)[FT], Unit<2> &encu) {
        constexpr int h = decltype(hh)::value;
        const uint32_t bc = stage_base(tile);
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const uint32_t smp = base + (2 * h + n) * 16 + col;
            const uint32_t sc = smp < P.M ? smp : P.M - 1;
            const uint32_t idx = sc - bc;  // position inside the staged 64 samples
#pragma unroll
            for (int t = 0; t < FT; ++t)
#pragma unroll
                for (int jb = 0; jb < 2; ++jb) {
                    const uint32_t piece = 8 * t + 4 * jb + q;  // float4 index inside the feature row
                    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (COMP || staged) {
                        // branch-free: the pieces past F read a valid staged piece and are zeroed by a select (`piece` depends
                        // on the lane, a branch here is a divergent one in front of every trunk)
                        const bool ok = 4 * piece + 4 <= P.F;
                        const f32x4 w = *reinterpret_cast<const f32x4 *>(stg + ((ok ? piece : 0u) * 64 + idx) * 4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = ok ? w[e] : 0.0f;
                    } else if (4 * piece + 4 <= P.F) {
                        v = P.feat_piece_major ? *reinterpret_cast<const f32x4 *>(P.feat + ((size_t)piece * P.M + sc) * 4)
                                               : *reinterpret_cast<const f32x4 *>(P.feat + (size_t)sc * P.F + 4 * piece);
                    }
                    fin[t].a[jb][n] = v;
                }
#pragma unroll
            for (int jb = 0; jb < 2; ++jb) {
                f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
                if (LIDAR) {  // (no view MLP: nothing reads the unit)
                } else if (COMP || staged) v = *reinterpret_cast<const f32x4 *>(stg + NLR_STAGE_ENC + (((2 * h + n) * 2 + jb) * 4 + q) * 4);
                else if (P.rgb) v = *reinterpret_cast<const f32x4 *>(P.enc + (size_t)(sc / P.S) * 32 + 16 * jb + 4 * q);
                encu.a[jb][n] = v;
            }
        }
    };

    NLR_STAMP(1);  // (tile prologue)
    // per-sample outputs of one half: density, class probabilities, intensity (class-major / channel-major stores: the 16
    // lanes of a row write 64 consecutive bytes)
    auto heads_out = [&](auto hh, const float (&raw)[2], const Unit<2> &lo) {
        constexpr int h = decltype(hh)::value;
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const uint32_t smp = base + (2 * h + n) * 16 + col;
            const bool valid = smp < P.M;
            if (q == 0 && valid) {
                P.density[smp] = nlr_softplus(raw[n] + P.density_bias);
            }
            if constexpr (HT > 0) {
                if (P.K > 0) {  // softmax over rows [0,K): 8 rows in this lane, the rest in the 3 other lanes of the column
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
                            if (valid && row < (int)P.K) P.sem[(size_t)row * P.M + smp] = e[jb][r] / s;
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
    };

    // ---- compositing mode: per half, the heads' outputs are turned into one segment record by NHP small pieces of VALU work
    struct HeadSt {
        Unit<2> lo;
        float raw[2], xr[2], ex[2], a[2], E[2], tp[2], wp[2], mx[2], sm[2], c[2];
        float acc[2][4];   // [row block][r]
    };
    float wpall[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // segment-local weight of this lane's sample in each column tile (kept for the rgb sums)
    // LIDAR: (t_k+1 - t_k) |d| and the last-sample flag of this lane's sample in each column tile, read from the staging area at the
    // start of the tile so that the next tile's inputs can be requested before the compositing pieces of the second half
    float tdd[4] = {0.0f, 0.0f, 0.0f, 0.0f}, tdf[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (LIDAR) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float *td = stg + NLR_STAGE_TD + 16 * g + col;
            tdd[g] = (td[64] - td[0]) * td[128];
            tdf[g] = td[192];
        }
    }
    constexpr int NHP = 35;
    auto head_piece = [&](auto hh, auto ii, HeadSt &st) {
        constexpr int h = decltype(hh)::value, I = decltype(ii)::value;
        if constexpr (I < 2) {  // raw density of the column (row 0 sits on the q = 0 lanes) -> every lane of the column; exp
            constexpr int n = I;
            st.xr[n] = nlr_q_sum(q == 0 ? st.raw[n] : 0.0f) + P.density_bias;
            st.ex[n] = expf(st.xr[n]);
        } else if constexpr (I < 4) {  // softplus (models.py:1116), density out, sigma * delta (render.py:176-180)
            constexpr int n = I - 2, g = 2 * h + n;
            const float sp = st.xr[n] > 20.0f ? st.xr[n] : log1pf(st.ex[n]);
            const uint32_t smp = base + g * 16 + col;
            if (q == 0 && smp < P.M) P.density[smp] = sp;
            const float *td = stg + NLR_STAGE_TD + 16 * g + col;  // staged t_k, t_k+1, |d|, last-sample flag of this lane's sample
            float a = sp * (LIDAR ? tdd[g] : (td[64] - td[0]) * td[128]);
            if ((LIDAR ? tdf[g] : td[192]) != 0.0f) a = INFINITY;  // opaque background: infinitely wide last interval
            st.a[n] = a;
        } else if constexpr (I == 4) {  // exclusive prefix of sigma*delta inside the segment (16-lane rows, then across the 2 tiles)
            const float i0 = nlr_row_incl_scan(st.a[0]);
            st.E[0] = nlr_row_shr1(i0);
        } else if constexpr (I == 5) {
            const float i1 = nlr_row_incl_scan(st.a[1]);
            st.E[1] = nlr_row_shr1(i1) + nlr_row_sum(st.a[0]);
        } else if constexpr (I < 8) {  // transmittance inside the segment
            constexpr int n = I - 6;
            st.tp[n] = __expf(-st.E[n]);  // (v_exp_f32: these weights only scale the value sums; the stored density keeps libm)
        } else if constexpr (I < 10) {  // alpha, segment-local weight
            constexpr int n = I - 8;
            st.wp[n] = (1.0f - __expf(-st.a[n])) * st.tp[n];
            wpall[2 * h + n] = st.wp[n];
        } else if constexpr (I < 14) {  // softmax over rows [0,K): running maximum of the masked logits
            constexpr int n = (I - 10) >> 1, jb = (I - 10) & 1;
            if constexpr (jb == 0) st.mx[n] = -INFINITY;
#pragma unroll
            for (int r = 0; r < 4; ++r) st.mx[n] = fmaxf(st.mx[n], (16 * jb + 4 * q + r) < (int)P.K ? st.lo.a[jb][n][r] : -INFINITY);
        } else if constexpr (I < 16) {
            constexpr int n = I - 14;
            st.mx[n] = nlr_q_max(st.mx[n]);
        } else if constexpr (I < 20) {  // sum of exp
            constexpr int n = (I - 16) >> 1, jb = (I - 16) & 1;
            if constexpr (jb == 0) st.sm[n] = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) st.sm[n] += (16 * jb + 4 * q + r) < (int)P.K ? __expf(st.lo.a[jb][n][r] - st.mx[n]) : 0.0f;
        } else if constexpr (I < 22) {  // weight / softmax denominator
            constexpr int n = I - 20;
            st.sm[n] = nlr_q_sum(st.sm[n]);
            st.c[n] = st.wp[n] / st.sm[n];
        } else if constexpr (I < 26) {  // w' p_c (exp again: cheaper than 16 live registers) and w' intensity in the intensity row
            constexpr int n = (I - 22) >> 1, jb = (I - 22) & 1;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * jb + 4 * q + r;
                const float x = st.lo.a[jb][n][r];
                const float v = row == (int)P.int_row ? x * st.wp[n] : (row < (int)P.K ? __expf(x - st.mx[n]) * st.c[n] : 0.0f);
                st.acc[jb][r] = n == 0 ? v : st.acc[jb][r] + v;
            }
        } else if constexpr (I < 34) {  // sum over the 16 samples of the row
            constexpr int jb = ((I - 26) >> 2) & 1, r = (I - 26) & 3;
            st.acc[jb][r] = nlr_row_sum(st.acc[jb][r]);
        } else {  // lanes col < 8 of each row hold one value each: rows 16*(col>>2) + 4q + (col&3)
            float v = st.acc[0][0];
#pragma unroll
            for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (col == 4 * jb + r) v = st.acc[jb][r];
            const uint32_t s0 = base + 32 * h;
            if (col < 8 && s0 < P.M) P.seg[(size_t)(s0 >> 5) * 32 + 16 * (col >> 2) + 4 * q + (col & 3)] = v;
        }
    };
    // one piece every HSTEP steps of view layers 0 and 1 of the same half (folded, layer 0 of a width-128 view MLP has 24 steps: fewer
    // than there are pieces)
    constexpr int SV0 = WT * (KB + 1) * 2, SV1 = WT * (WT + KB + 1) * 2;
    constexpr int HSTEP = (SV0 + SV1) / NHP;
    static_assert(!COMP || LIDAR || HSTEP >= 1, "not enough steps for the compositing pieces");

    if constexpr (!VIEW_F32) {
        // =================================================== bf16 view MLP ===================================================
        BT<4> hbe[KB + 1];  // [bottleneck (FOLD: hi part of h) | dir-enc] k-blocks of both halves (column tiles 2h, 2h+1 belong to half h)
        Unit<2> fin[FT], encu[2];
        auto trunk = [&](auto hh, Unit<2> &lo_out, float (&raw_out)[2]) {
            constexpr int h = decltype(hh)::value;
            constexpr int F0 = h * FR_HALF;
            load_inputs(hh, fin, encu[h]);
            if constexpr (LIDAR && h == 1) {  // every staged input of this tile is in registers: request the next tile's
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (tile + gridDim.x < ntiles) stage_issue(tile + gridDim.x);
            }
            float raw[2] = {0.0f, 0.0f};
            Unit<2> lo;
#pragma unroll
            for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                for (int n = 0; n < 2; ++n) lo.a[jb][n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if constexpr (X3) {
                // ---- density trunk + heads on split-bf16
                BT<2> fh[FT], fl[FT];
#pragma unroll
                for (int t = 0; t < FT; ++t) nlr_split_all<false, 0>(fh[t], fl[t], fin[t]);
                if constexpr (h == 0) NLR_STAMP(2);  // features split
                // h = relu(D0): the hi part goes straight into the view MLP's operand (column tiles of this half), the lo part stays local
                BT<2> dl[2];
                nlr_gemm<2, FT, 2, 2, 2, F0, 8>(
                    tp, [&](auto o, f32x4(&b)[2]) { bias_rows(lds_bias + OB_D0 + 32 * decltype(o)::value, b); },
                    [&](Unit<2> &u, auto g, auto j, const uint4 &f0, const uint4 &f1, const f32x4 &bj) {
                        constexpr int G = decltype(g)::value, J = decltype(j)::value;
                        nlr_mma_x3<G == 0, 0>(u.a[J], bj, f0, f1, fh[G], fl[G]);
                    },
                    [&](auto o, auto p, const Unit<2> &u) {
                        constexpr int O = decltype(o)::value, Pc = decltype(p)::value;
                        constexpr int n = Pc >> 2, jb = (Pc >> 1) & 1, pr = Pc & 1;
                        f32x2 xv = {u.a[jb][n][2 * pr], u.a[jb][n][2 * pr + 1]};
                        xv = __builtin_elementwise_max(xv, (f32x2){0.0f, 0.0f});
                        const bf16x2 hv = __builtin_convertvector(xv, bf16x2);
                        const bf16x2 lv = __builtin_convertvector(xv - __builtin_convertvector(hv, f32x2), bf16x2);
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            hbe[O].n[2 * h + n][4 * jb + 2 * pr + e] = hv[e];
                            dl[O].n[n][4 * jb + 2 * pr + e] = lv[e];
                        }
                    });
                if constexpr (h == 0) NLR_STAMP(3);  // D0
                // split-bf16 step against h: hi.hi, hi.lo, lo.hi per column tile (the order of nlr_mma_x3)
                auto mma_h = [&](Unit<2> &u, auto g, auto j, const uint4 &f0, const uint4 &f1, const f32x4 &bj) {
                    constexpr int G = decltype(g)::value, J = decltype(j)::value;
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        u.a[J][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(nlr_as<bf16x8>(f0), hbe[G].n[2 * h + n], G == 0 ? bj : u.a[J][n], 0, 0, 0);
                        u.a[J][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(nlr_as<bf16x8>(f0), dl[G].n[n], u.a[J][n], 0, 0, 0);
                        u.a[J][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(nlr_as<bf16x8>(f1), hbe[G].n[2 * h + n], u.a[J][n], 0, 0, 0);
                    }
                };
                // D2: the one unit that holds row 0, the raw density
                nlr_gemm<1, 2, 2, 2, 2, F0 + FR_D0, 1>(
                    tp, [&](auto, f32x4(&b)[2]) { bias_rows(lds_bias + OB_D2, b); }, mma_h,
                    [&](auto, auto, const Unit<2> &u) {
                        raw[0] = u.a[0][0][0];
                        raw[1] = u.a[0][1][0];
                    });
                if constexpr (h == 0) NLR_STAMP(4);  // D2
                if constexpr (HT > 0) {
                    BT<2> qh[HTA], ql[HTA];
                    nlr_gemm<HT, KB, 2, 2, 2, F0 + FR_D0 + FR_D2, 8>(
                        tp, [&](auto o, f32x4(&b)[2]) { bias_rows(lds_bias + OB_H1 + 32 * decltype(o)::value, b); }, mma_h,
                        [&](auto o, auto p, const Unit<2> &u) { nlr_split_piece<true, decltype(p)::value, 0>(qh[decltype(o)::value], ql[decltype(o)::value], u); });
                    if constexpr (h == 0) NLR_STAMP(5);  // H1
                    nlr_gemm<1, HT, 2, 2, 2, F0 + FR_D0 + FR_D2 + FR_H1, 1>(
                        tp, [&](auto o, f32x4(&b)[2]) { bias_rows(lds_bias + OB_H2, b); },
                        [&](Unit<2> &u, auto g, auto j, const uint4 &f0, const uint4 &f1, const f32x4 &bj) {
                            constexpr int G = decltype(g)::value, J = decltype(j)::value;
                            nlr_mma_x3<G == 0, 0>(u.a[J], bj, f0, f1, qh[G], ql[G]);
                        },
                        [&](auto, auto, const Unit<2> &u) { lo = u; });
                }
            } else {
                // ---- density trunk + heads on the exact-f32 MFMA (k-groups of 16 features)
                Unit<2> hid[2];
                nlr_gemm<2, 2 * FT, 2, 2, 1, F0, 1>(
                    tp, [&](auto o, f32x4(&b)[2]) { bias_rows(lds_bias + OB_D0 + 32 * decltype(o)::value, b); },
                    [&](Unit<2> &u, auto g, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
                        constexpr int G = decltype(g)::value, J = decltype(j)::value;
                        nlr_mma_f32<G == 0>(u.a[J], bj, f0, fin[G >> 1].a[G & 1]);
                    },
                    [&](auto o, auto, const Unit<2> &u) {
                        hid[decltype(o)::value] = u;
                        nlr_act_unit<true>(hid[decltype(o)::value]);
                    });
                Unit<2> hb[BW];
                nlr_gemm<BW, 4, 2, 2, 1, F0 + FR_D0, 1>(
                    tp, [&](auto o, f32x4(&b)[2]) { bias_rows(lds_bias + OB_D2 + 32 * decltype(o)::value, b); },
                    [&](Unit<2> &u, auto g, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
                        constexpr int G = decltype(g)::value, J = decltype(j)::value;
                        nlr_mma_f32<G == 0>(u.a[J], bj, f0, hid[G >> 1].a[G & 1]);
                    },
                    [&](auto o, auto, const Unit<2> &u) {
                        constexpr int O = decltype(o)::value;
                        if constexpr (O == 0) {
                            raw[0] = u.a[0][0][0];
                            raw[1] = u.a[0][1][0];
                        }
                        hb[O] = u;
                        nlr_pack_all<false, 2 * h>(hbe[O], u);
                    });
                if constexpr (HT > 0) {
                    Unit<2> hq[HTA];
                    nlr_gemm<HT, 2 * BW, 2, 2, 1, F0 + FR_D0 + FR_D2, 1>(
                        tp, [&](auto o, f32x4(&b)[2]) { bias_rows(lds_bias + OB_H1 + 32 * decltype(o)::value, b); },
                        [&](Unit<2> &u, auto g, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
                            constexpr int G = decltype(g)::value, J = decltype(j)::value;
                            nlr_mma_f32<G == 0>(u.a[J], bj, f0, hb[G >> 1].a[G & 1]);
                        },
                        [&](auto o, auto, const Unit<2> &u) {
                            hq[decltype(o)::value] = u;
                            nlr_act_unit<true>(hq[decltype(o)::value]);
                        });
                    nlr_gemm<1, 2 * HT, 2, 2, 1, F0 + FR_D0 + FR_D2 + FR_H1, 1>(
                        tp, [&](auto o, f32x4(&b)[2]) { bias_rows(lds_bias + OB_H2, b); },
                        [&](Unit<2> &u, auto g, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
                            constexpr int G = decltype(g)::value, J = decltype(j)::value;
                            nlr_mma_f32<G == 0>(u.a[J], bj, f0, hq[G >> 1].a[G & 1]);
                        },
                        [&](auto, auto, const Unit<2> &u) { lo = u; });
                }
            }
            if constexpr (h == 0) NLR_STAMP(6);  // H2
            if constexpr (COMP) {
                lo_out = lo;
                raw_out[0] = raw[0];
                raw_out[1] = raw[1];
            } else {
                heads_out(hh, raw, lo);
            }
            if constexpr (h == 0) NLR_STAMP(7);  // softmax + stores of half A
        };
        Unit<2> hlo;
        float hraw[2] = {0.0f, 0.0f};
        if constexpr (LIDAR) {
            // ---- LiDAR-only: per half trunk + heads, then the half's segment record (slots [29,32) are rows 29..31 of the heads'
            // output unit, which no class or intensity row reaches: head_piece writes 0 there)
            auto half = [&](auto hh) {
                trunk(hh, hlo, hraw);
                HeadSt hst;
                hst.lo = hlo;
                hst.raw[0] = hraw[0];
                hst.raw[1] = hraw[1];
                nlr_pend<0, NHP>([&](auto ii) {
                    head_piece(hh, ii, hst);
                    __builtin_amdgcn_sched_barrier(0);
                });
            };
            half(ic<0>{});
            half(ic<1>{});
            nlr_pad<(2 * FR_T) % NLR_CHUNK_FRAGS>(tp);
        } else {
        if (P.rgb == nullptr) {  // density / semantic / intensity only (uniform for the whole grid)
            trunk(ic<0>{}, hlo, hraw);
            nlr_skip<FR_T, FR_V0 + FR_V1>(tp);
            trunk(ic<1>{}, hlo, hraw);
            nlr_skip<FR_HALF + FR_T, FR_V0 + FR_V1>(tp);
            nlr_pad<F_HID % NLR_CHUNK_FRAGS>(tp);
            continue;
        }
        // ---- view MLP.  Layer 0 input = [bottleneck | enc]; layer 1 input = [x | bottleneck | enc] (skip concat,
        // models.py:1227-1228); the 27 dir-encoding features ride as one extra zero-padded 32-feature k-block.
        BT<4> x[WT], y[WT];
        Unit<2> cyh[2];
        // The last output unit of every layer is carried raw and packed behind the MFMAs of the next layer's first unit, whose
        // first k-groups do not read it.
        auto view01 = [&](auto hh) {
            constexpr int h = decltype(hh)::value;
            constexpr int F0 = h * FR_HALF + FR_T;
            HeadSt hst;  // (COMP) the half's heads, consumed piece by piece behind layer 0
            hst.lo = hlo;
            hst.raw[0] = hraw[0];
            hst.raw[1] = hraw[1];
            nlr_pack_all<false, 2 * h>(hbe[KB], encu[h]);
            Unit<2> cx;
            auto comp_bg = [&](auto st) {  // step `st` of view layers 0 + 1 of this half
                constexpr int IDX = decltype(st)::value;
                if constexpr (COMP && IDX % HSTEP == HSTEP / 2 && IDX / HSTEP < NHP) head_piece(hh, ic<IDX / HSTEP>{}, hst);
            };
            nlr_gemm_pipe<WT, KB + 1, 2, 2, F0, 8, 0, 1, true>(
                tp, cx, [&](auto o, f32x4(&b)[2]) { bias_rows(lds_bias + OB_V0 + 32 * decltype(o)::value, b); },
                [&](Unit<2> &u, auto g, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
                    constexpr int G = decltype(g)::value, J = decltype(j)::value;
                    nlr_mma_bf16<G == 0, 2 * h>(u.a[J], bj, f0, hbe[G]);
                },
                [&](auto o, auto p, const Unit<2> &u) { nlr_pack_piece<true, decltype(p)::value, 2 * h>(x[decltype(o)::value], u); }, nop,
                [&](auto st) { comp_bg(st); });
            nlr_gemm_pipe<WT, WT + KB + 1, 2, 2, F0 + FR_V0, 8, 8, (WT - 1) * 2, true>(
                tp, cyh[h], [&](auto o, f32x4(&b)[2]) { bias_rows(lds_bias + OB_V1 + 32 * decltype(o)::value, b); },
                [&](Unit<2> &u, auto g, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
                    constexpr int G = decltype(g)::value, J = decltype(j)::value;
                    if constexpr (G < WT) nlr_mma_bf16<G == 0, 2 * h>(u.a[J], bj, f0, x[G]);
                    else nlr_mma_bf16<false, 2 * h>(u.a[J], bj, f0, hbe[G - WT]);
                },
                [&](auto o, auto p, const Unit<2> &u) { nlr_pack_piece<true, decltype(p)::value, 2 * h>(y[decltype(o)::value], u); },
                [&](auto p) { nlr_pack_piece<true, decltype(p)::value, 2 * h>(x[WT - 1], cx); },
                [&](auto st) { comp_bg(ic<SV0 + decltype(st)::value>{}); });
        };
        trunk(ic<0>{}, hlo, hraw);
        NLR_STAMP(8);  // (unused)
        view01(ic<0>{});
        NLR_STAMP(9);  // V0 + V1 of half A
        trunk(ic<1>{}, hlo, hraw);
        view01(ic<1>{});
        NLR_STAMP(10);  // trunk + heads + V0 + V1 of half B
        if (staged) {  // every staged input of this tile has been read: request the next tile's (lands under the hidden layers)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (tile + gridDim.x < ntiles) stage_issue(tile + gridDim.x);
        }
        // hidden layers 2..depth-1 at full width (4 MFMAs per tape fragment), two per iteration (y -> x -> y) so that no
        // tile copies are needed.  The pending last unit of layer 1 is the concatenation of the two halves' units.
        Unit<4> cx4, cy4;
#pragma unroll
        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                cy4.a[jb][n] = cyh[0].a[jb][n];
                cy4.a[jb][2 + n] = cyh[1].a[jb][n];
            }
        uint32_t l = 2;
        for (; l + 1 < P.depth; l += 2) {
            const float *bl = lds_bias + OB_VL + (l - 2) * (WT * 32);
            nlr_gemm_pipe<WT, WT, 2, 4, F_HID, 16, 16, (WT - 1) * 2, true>(
                tp, cx4, [&](auto o, f32x4(&b)[2]) { bias_rows(bl + 32 * decltype(o)::value, b); },
                [&](Unit<4> &u, auto g, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
                    constexpr int G = decltype(g)::value, J = decltype(j)::value;
                    nlr_mma_bf16<G == 0, 0>(u.a[J], bj, f0, y[G]);
                },
                [&](auto o, auto p, const Unit<4> &u) { nlr_pack_piece<true, decltype(p)::value, 0>(x[decltype(o)::value], u); },
                [&](auto p) { nlr_pack_piece<true, decltype(p)::value, 0>(y[WT - 1], cy4); });
            nlr_gemm_pipe<WT, WT, 2, 4, F_HID, 16, 16, (WT - 1) * 2, true>(
                tp, cy4, [&](auto o, f32x4(&b)[2]) { bias_rows(bl + WT * 32 + 32 * decltype(o)::value, b); },
                [&](Unit<4> &u, auto g, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
                    constexpr int G = decltype(g)::value, J = decltype(j)::value;
                    nlr_mma_bf16<G == 0, 0>(u.a[J], bj, f0, x[G]);
                },
                [&](auto o, auto p, const Unit<4> &u) { nlr_pack_piece<true, decltype(p)::value, 0>(y[decltype(o)::value], u); },
                [&](auto p) { nlr_pack_piece<true, decltype(p)::value, 0>(x[WT - 1], cx4); });
        }
        NLR_STAMP(11);  // hidden layer pairs
        const bool odd = ((P.depth - 2) & 1) != 0;
        if (odd) {  // odd number of hidden layers: one more, serial epilogue, result moved back into y
            const float *bl = lds_bias + OB_VL + (l - 2) * (WT * 32);
            nlr_gemm_pipe<WT, WT, 2, 4, F_HID, 16, 16, (WT - 1) * 2, false>(
                tp, cx4, [&](auto o, f32x4(&b)[2]) { bias_rows(bl + 32 * decltype(o)::value, b); },
                [&](Unit<4> &u, auto g, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
                    constexpr int G = decltype(g)::value, J = decltype(j)::value;
                    nlr_mma_bf16<G == 0, 0>(u.a[J], bj, f0, y[G]);
                },
                [&](auto o, auto p, const Unit<4> &u) { nlr_pack_piece<true, decltype(p)::value, 0>(x[decltype(o)::value], u); },
                [&](auto p) { nlr_pack_piece<true, decltype(p)::value, 0>(y[WT - 1], cy4); });
#pragma unroll
            for (int t = 0; t < WT; ++t) y[t] = x[t];
        }
        Unit<4> out1;
        const float *brgb = lds_bias + OB_VL + (P.depth - 2) * (WT * 32);
        auto rgb_mma = [&](Unit<4> &u, auto g, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
            constexpr int G = decltype(g)::value, J = decltype(j)::value;
            nlr_mma_bf16<G == 0, 0>(u.a[J], bj, f0, y[G]);
        };
        if (odd) {
            nlr_gemm_pipe<1, WT, 1, 4, F_HID, 1, 0, 1, false>(
                tp, cx4, [&](auto, f32x4(&b)[2]) { bias_rows(brgb, b); }, rgb_mma, [&](auto, auto, const Unit<4> &u) { out1 = u; }, nop);
        } else {
            nlr_gemm_pipe<1, WT, 1, 4, F_HID, 1, 16, WT - 1, false>(
                tp, cx4, [&](auto, f32x4(&b)[2]) { bias_rows(brgb, b); }, rgb_mma, [&](auto, auto, const Unit<4> &u) { out1 = u; },
                [&](auto p) { nlr_pack_piece<true, decltype(p)::value, 0>(y[WT - 1], cy4); });
        }
        NLR_STAMP(12);  // rgb layer
        if constexpr (COMP) {  // sum over the segment of w' rgb -> slots 29..31 of the segment record
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float sum[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int n = 0; n < 2; ++n)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float z = P.rgb_premul * out1.a[0][2 * h + n][c] + P.rgb_bias;
                        const float sg = __frcp_rn(1.0f + __expf(-z));
                        sum[c] += (sg * (1.0f + 2.0f * P.rgb_padding) - P.rgb_padding) * wpall[2 * h + n];
                    }
                float v = 0.0f;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    sum[c] = nlr_row_sum(sum[c]);
                    if (col == c) v = sum[c];
                }
                const uint32_t s0 = base + 32 * h;
                if (q == 0 && col < 3 && s0 < P.M) P.seg[(size_t)(s0 >> 5) * 32 + 29 + col] = v;
            }
        } else if (q == 0) {  // rows 0..2 of the output unit sit on lanes 0..15
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const uint32_t smp = base + n * 16 + col;
                if (smp < P.M) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float z = P.rgb_premul * out1.a[0][n][c] + P.rgb_bias;
                        const float sg = 1.0f / (1.0f + expf(-z));
                        P.rgb[(size_t)c * P.M + smp] = sg * (1.0f + 2.0f * P.rgb_padding) - P.rgb_padding;
                    }
                }
            }
        }
        NLR_STAMP(13);  // rgb stores
        nlr_pad<F_END % NLR_CHUNK_FRAGS>(tp);
        if constexpr (!STAGE_SIG) {  // no hidden layer and no tape signal behind the request: the next tile's inputs are waited for here
            if (staged && P.depth == 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        NLR_STAMP(14);  // tape padding
#ifdef NLR_STAMPS
        if (tile + gridDim.x >= ntiles && threadIdx.x == 0 && blockIdx.x < 1024) {
            unsigned long long *dbg = nlr_stamp_buf + (size_t)blockIdx.x * NLR_NSTAMP;
            for (int i = 0; i < 15; ++i) dbg[i] = stamps[i];
            dbg[22] = rt0;
            dbg[23] = __builtin_amdgcn_s_memrealtime();
        }
#endif
        }  // !LIDAR
    } else {
        // =================================================== exact-f32 chain: each half runs the whole tape ======================
        auto pass = [&](auto hh) {
            constexpr int h = decltype(hh)::value;
            Unit<2> fin[FT], encu1;
            load_inputs(hh, fin, encu1);
            float raw[2] = {0.0f, 0.0f};
            Unit<2> lo;
#pragma unroll
            for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                for (int n = 0; n < 2; ++n) lo.a[jb][n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            Unit<2> hid[2];
            nlr_gemm<2, 2 * FT, 2, 2, 1, 0, 1>(
                tp, [&](auto o, f32x4(&b)[2]) { bias_rows(lds_bias + OB_D0 + 32 * decltype(o)::value, b); },
                [&](Unit<2> &u, auto g, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
                    constexpr int G = decltype(g)::value, J = decltype(j)::value;
                    nlr_mma_f32<G == 0>(u.a[J], bj, f0, fin[G >> 1].a[G & 1]);
                },
                [&](auto o, auto, const Unit<2> &u) {
                    hid[decltype(o)::value] = u;
                    nlr_act_unit<true>(hid[decltype(o)::value]);
                });
            Unit<2> hb[BW + 1];  // [bottleneck | dir-enc]
            nlr_gemm<BW, 4, 2, 2, 1, FR_D0, 1>(
                tp, [&](auto o, f32x4(&b)[2]) { bias_rows(lds_bias + OB_D2 + 32 * decltype(o)::value, b); },
                [&](Unit<2> &u, auto g, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
                    constexpr int G = decltype(g)::value, J = decltype(j)::value;
                    nlr_mma_f32<G == 0>(u.a[J], bj, f0, hid[G >> 1].a[G & 1]);
                },
                [&](auto o, auto, const Unit<2> &u) {
                    constexpr int O = decltype(o)::value;
                    if constexpr (O == 0) {
                        raw[0] = u.a[0][0][0];
                        raw[1] = u.a[0][1][0];
                    }
                    hb[O] = u;
                });
            if constexpr (HT > 0) {
                Unit<2> hq[HTA];
                nlr_gemm<HT, 2 * BW, 2, 2, 1, FR_D0 + FR_D2, 1>(
                    tp, [&](auto o, f32x4(&b)[2]) { bias_rows(lds_bias + OB_H1 + 32 * decltype(o)::value, b); },
                    [&](Unit<2> &u, auto g, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
                        constexpr int G = decltype(g)::value, J = decltype(j)::value;
                        nlr_mma_f32<G == 0>(u.a[J], bj, f0, hb[G >> 1].a[G & 1]);
                    },
                    [&](auto o, auto, const Unit<2> &u) {
                        hq[decltype(o)::value] = u;
                        nlr_act_unit<true>(hq[decltype(o)::value]);
                    });
                nlr_gemm<1, 2 * HT, 2, 2, 1, FR_D0 + FR_D2 + FR_H1, 1>(
                    tp, [&](auto o, f32x4(&b)[2]) { bias_rows(lds_bias + OB_H2, b); },
                    [&](Unit<2> &u, auto g, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
                        constexpr int G = decltype(g)::value, J = decltype(j)::value;
                        nlr_mma_f32<G == 0>(u.a[J], bj, f0, hq[G >> 1].a[G & 1]);
                    },
                    [&](auto, auto, const Unit<2> &u) { lo = u; });
            }
            heads_out(hh, raw, lo);
            if (P.rgb == nullptr) {
                nlr_pad<FR_T % NLR_CHUNK_FRAGS>(tp);
                return;
            }
            hb[BW] = encu1;
            Unit<2> x[WT], y[WT];
            nlr_gemm<WT, 2 * (BW + 1), 2, 2, 1, FR_T, 1>(
                tp, [&](auto o, f32x4(&b)[2]) { bias_rows(lds_bias + OB_V0 + 32 * decltype(o)::value, b); },
                [&](Unit<2> &u, auto g, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
                    constexpr int G = decltype(g)::value, J = decltype(j)::value;
                    nlr_mma_f32<G == 0>(u.a[J], bj, f0, hb[G >> 1].a[G & 1]);
                },
                [&](auto o, auto, const Unit<2> &u) {
                    x[decltype(o)::value] = u;
                    nlr_act_unit<true>(x[decltype(o)::value]);
                });
            nlr_gemm<WT, 2 * (WT + BW + 1), 2, 2, 1, FR_T + FR_V0, 1>(
                tp, [&](auto o, f32x4(&b)[2]) { bias_rows(lds_bias + OB_V1 + 32 * decltype(o)::value, b); },
                [&](Unit<2> &u, auto g, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
                    constexpr int G = decltype(g)::value, J = decltype(j)::value;
                    if constexpr (G < 2 * WT) nlr_mma_f32<G == 0>(u.a[J], bj, f0, x[G >> 1].a[G & 1]);
                    else nlr_mma_f32<false>(u.a[J], bj, f0, hb[(G - 2 * WT) >> 1].a[G & 1]);
                },
                [&](auto o, auto, const Unit<2> &u) {
                    y[decltype(o)::value] = u;
                    nlr_act_unit<true>(y[decltype(o)::value]);
                });
            for (uint32_t l = 2; l < P.depth; ++l) {
                const float *bl = lds_bias + OB_VL + (l - 2) * (WT * 32);
                nlr_gemm<WT, 2 * WT, 2, 2, 1, F_HID, 1>(
                    tp, [&](auto o, f32x4(&b)[2]) { bias_rows(bl + 32 * decltype(o)::value, b); },
                    [&](Unit<2> &u, auto g, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
                        constexpr int G = decltype(g)::value, J = decltype(j)::value;
                        nlr_mma_f32<G == 0>(u.a[J], bj, f0, y[G >> 1].a[G & 1]);
                    },
                    [&](auto o, auto, const Unit<2> &u) {
                        x[decltype(o)::value] = u;
                        nlr_act_unit<true>(x[decltype(o)::value]);
                    });
#pragma unroll
                for (int t = 0; t < WT; ++t) y[t] = x[t];
            }
            Unit<2> out1;
            nlr_gemm<1, 2 * WT, 1, 2, 1, F_HID, 1>(
                tp, [&](auto, f32x4(&b)[2]) { bias_rows(lds_bias + OB_VL + (P.depth - 2) * (WT * 32), b); },
                [&](Unit<2> &u, auto g, auto j, const uint4 &f0, const uint4 &, const f32x4 &bj) {
                    constexpr int G = decltype(g)::value, J = decltype(j)::value;
                    nlr_mma_f32<G == 0>(u.a[J], bj, f0, y[G >> 1].a[G & 1]);
                },
                [&](auto, auto, const Unit<2> &u) { out1 = u; });
            if (q == 0) {
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const uint32_t smp = base + (2 * h + n) * 16 + col;
                    if (smp < P.M) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const float z = P.rgb_premul * out1.a[0][n][c] + P.rgb_bias;
                            const float sg = 1.0f / (1.0f + expf(-z));
                            P.rgb[(size_t)c * P.M + smp] = sg * (1.0f + 2.0f * P.rgb_padding) - P.rgb_padding;
                        }
                    }
                }
            }
            nlr_pad<F_END % NLR_CHUNK_FRAGS>(tp);
        };
        pass(ic<0>{});
        pass(ic<1>{});
        // Both halves have read their staged inputs: fetch the next tile's.  (Round 2 staged only a workgroup's FIRST tile on this
        // path, so with more tiles than workgroups - more than 65 536 samples on 256 CUs - every later tile of a workgroup was
        // evaluated on its first tile's features: found by the full-size parity run, tests/test_fullsize_parity.py.)  Nothing
        // overlaps this wait; the exact-f32 chain is the reference-grade mode, not the fast one.
        if (staged && tile + gridDim.x < ntiles) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            stage_issue(tile + gridDim.x);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    }  // tile loop
    // the read-ahead DMA must not outlive the workgroup's LDS allocation
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}


// One explicit instance per translation unit (nlr_mlp_inst.hip is compiled once per (WT, HT, PREC, COMP) by the Makefile:
// the fully unrolled GEMM chain is slow to compile, so the instances build in parallel).
#define NLR_MLP_LAUNCH_NAME2(wt, ht, pr, cm) nlr_mlp_launch_##wt##_##ht##_##pr##_##cm
#define NLR_MLP_LAUNCH_NAME(wt, ht, pr, cm) NLR_MLP_LAUNCH_NAME2(wt, ht, pr, cm)
#define NLR_MLP_DECLARE(wt, ht, pr, cm) void NLR_MLP_LAUNCH_NAME(wt, ht, pr, cm)(const MlpParams &P, dim3 grid, hipStream_t st)

