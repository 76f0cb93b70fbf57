// The weight tape of the fused NerfMLP kernels (inference: nlr_mlp_kernel.h, training: nlr_mlp_train.hip), stated once: its constants,
// the fragment layout, the stacked heads and the tile programs.  Plain C++ (no HIP): the kernels evaluate the program tables at compile
// time, the host builders (build_level in nlr_api.hip, plan_build in nlr_mlp_train.hip) walk the same layout and evaluate the same tables
// at run time, and refuse to hand out a tape or a bias block whose length differs from what the kernel will consume.
//
// One fragment = 1 KiB = 64 lanes x 16 B, the A operand of one MFMA step for 16 output rows; lane = (m = lane & 15, q = lane >> 4).
//   bf16 (v_mfma_f32_16x16x32_bf16): rows 16R + m, k-group g of 32 input features: element e = W[16R + m][32g + 16(e>>2) + 4q + (e&3)],
//        the k order in which two 16-row accumulator tiles of the previous layer, converted pairwise, form the B operand
//   f32  (v_mfma_f32_16x16x4_f32, 4 k-steps per fragment): rows 16R + m, k-group g of 16 features: element e = W[16R + m][16g + 4q + e]
// GEMM order on the tape: output unit o (32 rows) -> k-group g -> row block j (R = 2o + j; RH = 1: R = o, only the first 16 rows of the
// unit exist) [-> hi, lo fragment of the split-bf16 form].  GEMMs follow each other without padding; the end of a tile's program is
// padded to a whole chunk, and NLR_TAPE_SLACK_CHUNKS zero chunks follow the last program of a buffer.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/nerflidar_hip.h"

#define NLR_FRAG_BYTES 1024                                 // one fragment
#define NLR_CHUNK_FRAGS 32                                  // fragments per chunk (one buffer of the kernels' LDS ring)
#define NLR_CHUNK_BYTES (NLR_CHUNK_FRAGS * NLR_FRAG_BYTES)  // 32 KiB
#define NLR_CHUNK_BF16 (NLR_CHUNK_BYTES / 2)                // bf16 elements per chunk (the training tapes are addressed in elements)
#define NLR_TAPE_SLACK_CHUNKS 3                             // the kernels prefetch up to 3 chunks past the end of a tape

// What a host builder made (fragments of a tape, floats of a bias block) against what the kernel's program will consume: false, and a
// message naming both numbers, when they differ (nlr_tape_check in nlr_common.h turns that into NLR_ERR_UNSUPPORTED).
inline bool nlr_tape_matches(const char *what, size_t built, size_t program, char *msg, size_t msg_size) {
    if (built == program) return true;
    snprintf(msg, msg_size, "%s: the host built %zu, the kernel's program has %zu", what, built, program);
    return false;
}

// ---- dense row-major matrix over weights (float, absent = 0) or over flat-parameter indices (int32, absent = -1) ---------------------
template <class T, int ABSENT>
struct TapeMat {
    std::vector<T> a;
    uint32_t rows = 0, cols = 0;
    TapeMat() {}
    TapeMat(uint32_t r, uint32_t c) : a((size_t)r * c, (T)ABSENT), rows(r), cols(c) {}
    T &at(uint32_t r, uint32_t c) { return a[(size_t)r * cols + c]; }
    T get(uint32_t r, uint32_t c) const { return (r < rows && c < cols) ? a[(size_t)r * cols + c] : (T)ABSENT; }
    void paste(uint32_t r0, uint32_t c0, const TapeMat &m) {  // m at (r0, c0)
        for (uint32_t r = 0; r < m.rows; ++r)
            for (uint32_t c = 0; c < m.cols; ++c) at(r0 + r, c0 + c) = m.a[(size_t)r * m.cols + c];
    }
    TapeMat slice(uint32_t r0, uint32_t nr, uint32_t c0, uint32_t nc) const {  // [nr, nc] from (r0, c0); absent outside this matrix
        TapeMat m(nr, nc);
        for (uint32_t r = 0; r < nr; ++r)
            for (uint32_t c = 0; c < nc; ++c) m.at(r, c) = get(r0 + r, c0 + c);
        return m;
    }
    TapeMat t() const {
        TapeMat m(cols, rows);
        for (uint32_t r = 0; r < rows; ++r)
            for (uint32_t c = 0; c < cols; ++c) m.at(c, r) = a[(size_t)r * cols + c];
        return m;
    }
};
template <class T, int ABSENT>
struct TapeLinear {  // one Linear layer: weight [out, in] and bias [out]
    TapeMat<T, ABSENT> w;
    std::vector<T> b;
};

// ---- the walk of one GEMM: frag(v, n) receives every fragment in tape order, n = 64 * KW / 4 elements in lane order ------------------
// out_pad: rows padded to whole units of 32 (RH = 2) or to 16 (RH = 1, a single unit); in_pad: input features padded to whole k-groups
// of KW = 32 (bf16 paths) or 16 (exact f32).
template <class T, int ABSENT, class Frag>
void nlr_tape_walk(const TapeMat<T, ABSENT> &w, uint32_t out_pad, uint32_t in_pad, uint32_t KW, uint32_t RH, Frag &&frag) {
    const uint32_t OT = RH == 2 ? out_pad / 32 : 1, KG = in_pad / KW, EL = KW / 4;
    T v[64 * 8];
    for (uint32_t o = 0; o < OT; ++o)
        for (uint32_t g = 0; g < KG; ++g)
            for (uint32_t j = 0; j < RH; ++j) {
                const uint32_t R = RH == 2 ? 2 * o + j : o;
                for (uint32_t lane = 0; lane < 64; ++lane)
                    for (uint32_t e = 0; e < EL; ++e)
                        v[lane * EL + e] = w.get(16 * R + (lane & 15), KW * g + 16 * (e >> 2) + 4 * (lane >> 4) + (e & 3));
                frag((const T *)v, 64 * EL);
            }
}

// ---- the heads as two stacked GEMMs: h1 = [sem0 ; int0] (64 hidden rows each), h2 = [sem2 | 0 ; 0 | int2] block-diagonal into ONE 32-row
// unit, the intensity row behind the K class rows.  An absent head takes no rows; a head given as empty layers (the inference path's
// no_sem_layer pass-through, filled in by its caller) keeps its rows absent.
template <class T, int ABSENT>
struct TapeHeads {
    TapeMat<T, ABSENT> h1, h2;
    std::vector<T> b1, b2;
};
template <class T, int ABSENT>
TapeHeads<T, ABSENT> nlr_tape_heads(uint32_t WB, uint32_t K, const TapeLinear<T, ABSENT> *sem0, const TapeLinear<T, ABSENT> *sem2,
                                    const TapeLinear<T, ABSENT> *int0, const TapeLinear<T, ABSENT> *int2) {
    TapeHeads<T, ABSENT> h;
    const uint32_t HH = (sem0 ? 64 : 0) + (int0 ? 64 : 0);
    h.h1 = TapeMat<T, ABSENT>(HH, WB), h.h2 = TapeMat<T, ABSENT>(32, HH);
    h.b1.assign(HH, (T)ABSENT), h.b2.assign(32, (T)ABSENT);
    uint32_t r0 = 0;
    auto put = [&](const TapeLinear<T, ABSENT> &l0, const TapeLinear<T, ABSENT> &l2, uint32_t row) {  // hidden rows r0.., outputs row..
        h.h1.paste(r0, 0, l0.w);
        h.h2.paste(row, r0, l2.w);
        for (size_t i = 0; i < l0.b.size(); ++i) h.b1[r0 + i] = l0.b[i];
        for (size_t i = 0; i < l2.b.size(); ++i) h.b2[row + i] = l2.b[i];
        r0 += 64;
    };
    if (sem0) put(*sem0, *sem2, 0);
    if (int0) put(*int0, *int2, K);
    return h;
}

// ---- the tile programs: fragments per GEMM, positions derived from them, offsets (floats) of the bias block --------------------------
// WT = view width / 32, BW = bottleneck / 32, FT = grid-feature k-blocks of 32, HT = head hidden units of 32 (0, 2 or 4).
// TF: fragments per step in the trunk / heads (2 = split bf16); TK / VK: k-groups per 32 input features in the trunk / heads and in the view
// MLP (2 = exact f32); KB: k-blocks of the vector the heads and the view layers read; D2U: output units of density_layer.2.
// Bias block: b_d0 | b_d2 (D2U units) | b_h1 | b_h2 (one unit, also without heads) | view 0 | view 1 | view 2.. | rgb (one unit).
struct TapeGemms {
    int FR_D0, FR_D2, FR_H1, FR_H2, FR_T;  // FR_T: trunk + heads
    int FR_V0, FR_V1, FR_HL, FR_RGB;       // view layers 0 and 1, one hidden view layer, rgb_layer
    int OB_D0, OB_D2, OB_H1, OB_H2, OB_V0, OB_V1, OB_VL;
    constexpr int bias_end(int depth) const { return OB_VL + (depth - 2) * (OB_VL - OB_V1) + 32; }
};
constexpr TapeGemms nlr_tape_gemms(int WT, int BW, int FT, int HT, int TF, int TK, int VK, int KB, int D2U) {
    TapeGemms g = {};
    g.FR_D0 = 2 * (FT * TK) * 2 * TF, g.FR_D2 = D2U * (2 * TK) * 2 * TF;
    g.FR_H1 = HT * (KB * TK) * 2 * TF, g.FR_H2 = (HT * TK) * 2 * TF;
    g.FR_T = g.FR_D0 + g.FR_D2 + g.FR_H1 + g.FR_H2;
    g.FR_V0 = WT * ((KB + 1) * VK) * 2, g.FR_V1 = WT * ((WT + KB + 1) * VK) * 2;
    g.FR_HL = WT * (WT * VK) * 2, g.FR_RGB = WT * VK;
    g.OB_D0 = 0, g.OB_D2 = 64, g.OB_H1 = g.OB_D2 + D2U * 32, g.OB_H2 = g.OB_H1 + HT * 32, g.OB_V0 = g.OB_H2 + 32;
    g.OB_V1 = g.OB_V0 + WT * 32, g.OB_VL = g.OB_V1 + WT * 32;
    return g;
}

// Inference (nlr_mlp_kernel<WT, BW, FT, HT, PREC, CM>).  bf16 view MLP: [T V0 V1 | T V0 V1 | hidden x (depth - 2) | RGB] (the trunk + heads T
// and view layers 0 / 1 run once per 32-sample half); exact-f32 chain: [T V0 V1 | hidden.. | RGB], consumed once per half; LiDAR-only
// compositing (CM = 2): [T | T] on a tape of its own.  NLR_PREC_FAST folds density_layer.2 into its consumers (KB = 2, D2U = 1).
struct MlpProgram : TapeGemms {
    int KB, D2U;
    int FR_HALF, F_HID, F_END;  // one half; position of the hidden layers; end of the program without them
    bool LIDAR;
    constexpr int frags(int depth) const { return LIDAR ? 2 * FR_T : F_END + (depth - 2) * FR_HL; }
};
constexpr MlpProgram nlr_mlp_program(int WT, int BW, int FT, int HT, int PREC, int CM) {
    const bool X3 = PREC == NLR_PREC_FAST, VIEW_F32 = PREC == NLR_PREC_F32, LIDAR = CM == 2;
    const int KB = X3 ? 2 : BW, D2U = X3 ? 1 : BW;
    const TapeGemms g = nlr_tape_gemms(WT, BW, FT, HT, X3 ? 2 : 1, X3 ? 1 : 2, VIEW_F32 ? 2 : 1, KB, D2U);
    const int half = LIDAR ? g.FR_T : g.FR_T + g.FR_V0 + g.FR_V1, hid = VIEW_F32 ? half : 2 * half;
    return {g, KB, D2U, half, hid, hid + g.FR_RGB, LIDAR};
}

// Training (nlr_mlp_train_kernel<WT, BW, FT, HT, BWD, VIEW>), plain bf16, one wave = 32 samples.
//   forward:  D0 D2 [H1 H2] (V0 V1 hidden.. RGB)
//   backward: (RGB^T hidden^T.. V1a^T) H2^T BIG D2^T D0^T with BIG = [V1 skip^T | V0^T | H1^T | e_0] (BW units x (2 WT + HT + 1) k-groups)
// The parts in brackets exist with the view MLP only (VIEW; without it BIG shrinks to [H1^T | e_0] and WT does not enter the backward).
struct TrainProgram : TapeGemms {
    int FF_HID, FF_END;
    int BR_RGB, BR_V1A, BR_H2, BR_BIG, BR_D2, BR_D0;
    int BF_V1A, BF_H2, BF_BIG, BF_D2, BF_D0, BF_END;  // positions without the hidden layers (whole chunks between RGB^T and V1a^T)
    bool VIEW;
    constexpr int fwd_frags(int depth) const { return VIEW ? FF_END + (depth - 2) * FR_HL : FR_T; }
    constexpr int bwd_frags(int depth) const { return BF_END + (VIEW ? (depth - 2) * FR_HL : 0); }
};
constexpr TrainProgram nlr_train_program(int WT, int BW, int FT, int HT, bool VIEW) {
    const TapeGemms g = nlr_tape_gemms(WT, BW, FT, HT, 1, 1, 1, BW, BW);
    TrainProgram p = {g};
    p.VIEW = VIEW;
    p.FF_HID = g.FR_T + g.FR_V0 + g.FR_V1, p.FF_END = p.FF_HID + g.FR_RGB;
    const int VW = VIEW ? WT : 0;
    p.BR_RGB = VW * 1 * 2, p.BR_V1A = VW * VW * 2, p.BR_H2 = HT * 1 * 2, p.BR_BIG = BW * (2 * VW + HT + 1) * 2, p.BR_D2 = 2 * BW * 2;
    p.BR_D0 = FT * 2 * 2;
    p.BF_V1A = p.BR_RGB, p.BF_H2 = p.BF_V1A + p.BR_V1A, p.BF_BIG = p.BF_H2 + p.BR_H2, p.BF_D2 = p.BF_BIG + p.BR_BIG;
    p.BF_D0 = p.BF_D2 + p.BR_D2, p.BF_END = p.BF_D0 + p.BR_D0;
    return p;
}
