// The plan of the fused training NerfMLP (header section 6b), shared by the forward / backward chains (nlr_mlp_train.hip) and the
// weight-gradient kernel (nlr_mlp_wgrad.hip).
#pragma once
#include <vector>

#include "nlr_common.h"

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
    std::vector<uint32_t> offs;  // flat offsets: see nlr_train_param_layout
};
