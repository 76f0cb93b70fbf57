// The Linears of one object network (ObjMLP, ZI/models.py:881-950 as configured for a class), stated once: their shapes, the input
// blocks each one takes, their places in the kernel's LDS image, in the flat parameter buffer of the training form and in the columns
// of acts / gacts.  Plain C++ (no HIP).  nlr_objects.hip makes the ObjNet offsets of the render and training kernels from this table,
// nlr_objects_train.h the flat-buffer layouts and the ObjTrainLin records of the weight-gradient kernels; nothing else states a shape.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "../../include/nerflidar_hip.h"

#ifdef __HIPCC__
#define NLR_OBJ_HD __host__ __device__
#else
#define NLR_OBJ_HD
#endif

#define NLR_OBJ_MAX_CLASSES 8
#define NLR_OBJ_MAX_DEPTH 4
#define NLR_OBJ_MAX_DEG 4
#define NLR_OBJ_LINEARS (2 + NLR_OBJ_MAX_DEPTH + 1)  // density_layer.0, density_layer.2, lin_second_stage_0..D-1, rgb_layer
#define NLR_OBJ_WMAX 20480                           // floats of LDS for the weight image (80 KiB)

// Columns of the training form's saved tensors, for the kernels and the host alike:
//   acts  (every layer's input):               [grid | hidden 64 | bottleneck | dir enc | view 0 .. D-1]
//   gacts (every Linear's pre-activation grad): [hidden 64 | bottleneck | view 0 .. D-1 | rgb 4]
struct ObjCols {
    uint32_t cH0, cBOT, cDE, cV, aw;
    uint32_t gBOT, gV, gRGB, gw;
};
NLR_OBJ_HD inline ObjCols nlr_obj_cols(uint32_t n_grid, uint32_t BW, uint32_t DE, uint32_t D, uint32_t W) {
    ObjCols c;
    c.cH0 = n_grid, c.cBOT = c.cH0 + 64, c.cDE = c.cBOT + BW, c.cV = c.cDE + DE, c.aw = c.cV + D * W;
    c.gBOT = 64, c.gV = c.gBOT + BW, c.gRGB = c.gV + D * W, c.gw = c.gRGB + 4;
    return c;
}

// An input block of a Linear: `n` inputs from input column `wcol` on.  They are columns `src`.. of acts, or, for the two halves of the
// track's latent code (never stored per sample), entries `src`.. of the code.
enum ObjInKind { OBJ_IN_GRID, OBJ_IN_LAT_SHAPE, OBJ_IN_PREV, OBJ_IN_BOT, OBJ_IN_DE, OBJ_IN_LAT_TEX };
struct ObjInput {
    uint32_t kind, n, wcol, src;
    bool latent() const { return kind == OBJ_IN_LAT_SHAPE || kind == OBJ_IN_LAT_TEX; }
};
struct ObjLinear {
    const char *name;
    uint32_t n_out, n_in, outp;  // nn.Linear [n_out, n_in]; outputs padded to outp (64 / 64 / 32 / 4) in the image
    uint32_t n_inputs;
    ObjInput in[5];              // in input order
    uint32_t g_col;              // first column of its pre-activation gradient in gacts
    uint32_t w_off, b_off;       // flat buffer: weight [n_out, n_in] row-major, then bias [n_out], Linear after Linear
    uint32_t img_w, img_b;       // image: [n_in][outp] of every Linear, then the biases [outp] of every Linear
};
struct ObjLayers {
    uint32_t n_grid, lat_shape, lat_tex, lat_tex_off, BW, W, D, skip, deg, DE;
    ObjCols col;
    uint32_t n_lin;
    ObjLinear lin[NLR_OBJ_LINEARS];
    uint32_t n_params, img_floats;  // lengths of the flat buffer and of the image
};

// The table of one class.  false and a message when the class lies outside the kernels' envelope (`who` names the entry point in the
// one message that three of them give).
inline bool nlr_obj_layers(const NlrObjClassDesc &cd, const char *who, uint32_t cls, ObjLayers &t, char *msg, size_t msg_size) {
    const NlrMlpDesc &md = cd.mlp;
#define OBJ_REQ(cond, ...)                    \
    if (!(cond)) {                            \
        snprintf(msg, msg_size, __VA_ARGS__); \
        return false;                         \
    }
    OBJ_REQ(!md.disable_rgb, "objects_create: class %u: an ObjMLP has an rgb branch", cls);
    OBJ_REQ(md.bottleneck_width >= 1 && md.bottleneck_width <= 64, "objects_create: bottleneck_width %u outside [1,64]", md.bottleneck_width);
    OBJ_REQ(md.net_width_viewdirs >= 1 && md.net_width_viewdirs <= 32, "objects_create: net_width_viewdirs %u outside [1,32]", md.net_width_viewdirs);
    OBJ_REQ(md.net_depth_viewdirs >= 1 && md.net_depth_viewdirs <= NLR_OBJ_MAX_DEPTH, "%s: net_depth_viewdirs %u outside [1,%d]", who,
            md.net_depth_viewdirs, NLR_OBJ_MAX_DEPTH);
    OBJ_REQ(md.deg_view <= NLR_OBJ_MAX_DEG, "objects_create: deg_view %u > %d", md.deg_view, NLR_OBJ_MAX_DEG);
    OBJ_REQ(!md.re_weights, "objects_create: ObjMLP runs without erf re-weighting (models.py:137)");
    t = ObjLayers{};
    const uint32_t lat = cd.latent_size;
    t.n_grid = md.grid.num_levels * md.grid.level_dim;
    t.lat_shape = lat ? (cd.split_latent ? lat / 2 : lat) : 0;
    t.lat_tex = (lat && cd.split_latent) ? lat - lat / 2 : 0;
    t.lat_tex_off = lat / 2;
    t.BW = md.bottleneck_width, t.W = md.net_width_viewdirs, t.D = md.net_depth_viewdirs, t.skip = md.skip_layer_dir;
    t.deg = md.deg_view, t.DE = 3 + 6 * md.deg_view;
    t.col = nlr_obj_cols(t.n_grid, t.BW, t.DE, t.D, t.W);
    auto add = [&t](const char *name, uint32_t n_out, uint32_t outp, uint32_t g_col) -> ObjLinear & {
        ObjLinear &L = t.lin[t.n_lin++];
        L.name = name, L.n_out = n_out, L.outp = outp, L.g_col = g_col;
        return L;
    };
    auto input = [](ObjLinear &L, uint32_t kind, uint32_t n, uint32_t src) {  // the next n input columns (an empty block is no block)
        if (!n) return;
        L.in[L.n_inputs++] = ObjInput{kind, n, L.n_in, src};
        L.n_in += n;
    };
    // the concatenated input of the view MLP: [bottleneck | dir enc | texture half], models.py:1190-1234
    auto concat = [&](ObjLinear &L) {
        input(L, OBJ_IN_BOT, t.BW, t.col.cBOT);
        input(L, OBJ_IN_DE, t.DE, t.col.cDE);
        input(L, OBJ_IN_LAT_TEX, t.lat_tex, t.lat_tex_off);
    };
    {
        ObjLinear &L = add("density_layer.0", 64, 64, 0);
        input(L, OBJ_IN_GRID, t.n_grid, 0);
        input(L, OBJ_IN_LAT_SHAPE, t.lat_shape, 0);
    }
    input(add("density_layer.2", t.BW, 64, t.col.gBOT), OBJ_IN_PREV, 64, t.col.cH0);
    for (uint32_t i = 0; i < t.D; ++i) {  // layer 0 takes the concatenation, layer skip + 1 takes it again behind layer skip's outputs
        ObjLinear &L = add("lin_second_stage", t.W, 32, t.col.gV + i * t.W);
        if (i > 0) input(L, OBJ_IN_PREV, t.W, t.col.cV + (i - 1) * t.W);
        if (i == 0 || i - 1 == t.skip) concat(L);
    }
    {
        ObjLinear &L = add("rgb_layer", 3, 4, t.col.gRGB);
        input(L, OBJ_IN_PREV, t.W, t.col.cV + (t.D - 1) * t.W);
        if (t.D - 1 == t.skip) concat(L);
    }
    for (uint32_t i = 0; i < t.n_lin; ++i) {
        ObjLinear &L = t.lin[i];
        L.w_off = t.n_params;
        L.b_off = L.w_off + L.n_out * L.n_in;
        t.n_params = L.b_off + L.n_out;
        L.img_w = t.img_floats;
        t.img_floats += L.n_in * L.outp;
    }
    for (uint32_t i = 0; i < t.n_lin; ++i) {
        t.lin[i].img_b = t.img_floats;
        t.img_floats += t.lin[i].outp;
    }
    OBJ_REQ(t.img_floats <= NLR_OBJ_WMAX, "objects_create: class %u needs %zu floats of LDS for its weights, the kernel holds %d", cls,
            (size_t)t.img_floats, NLR_OBJ_WMAX);
#undef OBJ_REQ
    return true;
}
