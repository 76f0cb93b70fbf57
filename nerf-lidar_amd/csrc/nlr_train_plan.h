// The plan of the fused training NerfMLP (header section 6b), shared by the forward / backward chains (nlr_mlp_train.hip) and the
// weight-gradient kernel (nlr_mlp_wgrad.hip).  `linears` is the ONE description of the network: which Linear layers exist, in what
// order, which columns of acts / gacts each reads and writes, which reduce over the colour rows only.  The tapes, the bias block, the
// weight-gradient jobs and (through nlr_train_linear_table) the host-side GEMMs are all derived from it.
#pragma once
#include <vector>

#include "nlr_common.h"

// Columns of acts [M, act_w] = [hid 64 | bottleneck WB | head hidden 32 HT | x_0 .. x_{D-1}, W each]; gacts [M, act_w + 64] holds the
// gradient of every pre-activation in the same columns, then [d head outputs 32 | d rgb_layer outputs 32] at c_lo / c_o.
struct TrainCols {
    uint32_t c_hid, c_hbe, c_q, c_x, c_lo, c_o;  // c_lo = act_w
};
constexpr TrainCols nlr_train_cols(uint32_t W, uint32_t WB, uint32_t HT, uint32_t D) {
    const uint32_t c_hbe = 64, c_q = c_hbe + WB, c_x = c_q + 32 * HT, act_w = c_x + D * W;
    return {0, c_hbe, c_q, c_x, act_w, act_w + 32};
}

enum { NLR_TRAIN_SRC_ACTS = 0, NLR_TRAIN_SRC_FEATURES = 1, NLR_TRAIN_SRC_ENC = 2 };
struct TrainBlock {  // columns [col, col + n) of acts, of the grid features or of the per-ray direction encoding
    uint32_t src, col, n;
};
struct TrainLinear {  // one Linear, in flat-parameter order: y = W [in_0 | in_1 | ..] + b
    uint32_t g_col, n_out;  // its pre-activation gradient: gacts columns [g_col, g_col + n_out)
    uint32_t o_off;         // columns in front of g_col that belong to another Linear of the same 32-column unit (the intensity row
                            // sits behind the K semantic rows): g_col - o_off is 16-byte aligned
    TrainBlock in[3];       // input blocks, in the order of the weight's columns
    uint32_t n_in;          // blocks used
    uint32_t color;         // 1: lin_second_stage_* and rgb_layer, which see the rows with colour supervision only
    uint32_t w_off, b_off;  // offsets (floats) of weight [n_out, sum of in[].n] and bias inside the flat parameter buffer
};
#define NLR_TRAIN_TABLE_ROW 16  // uint32 per Linear of nlr_train_linear_table

struct NlrTrainPlan {
    uint32_t F, W, WB, HT, D, K, E, int_row, act_w, n_params, cus;  // E = 3 + 6 deg_view: columns of enc the view layers read
    bool sem, inten;
    float density_bias, rgb_premul, rgb_bias, rgb_padding;
    int32_t *fidx = nullptr, *bidx = nullptr, *biasidx = nullptr;
    uint32_t fn = 0, bn = 0, biasn = 0;  // elements nlr_train_pack gathers: the full tape, then the trunk-and-heads tape behind it
    // [f0, f0 + f0n) / [f1, f1 + f1n): the full tape and the trunk-and-heads tape (rows without colour supervision) inside ftape;
    // b0 .. likewise inside btape.  All in bf16 elements, multiples of one 32 KiB chunk.
    uint32_t f0n = 0, f1 = 0, f1n = 0, b0n = 0, b1 = 0, b1n = 0;
    __bf16 *ftape = nullptr, *btape = nullptr;
    float *bias = nullptr;
    std::vector<TrainLinear> linears;
};
