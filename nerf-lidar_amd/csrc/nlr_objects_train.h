// Training form of the dynamic-object branch (header section 7e).  This file is the tail of nlr_objects.hip - one translation unit:
// the kernels below go through the box-frame map, the owner / scan / scatter kernels, the ObjNet image and the obj_* layer helpers of
// that file, on the plan's own NlrObjects (laid out and allocated by obj_layout; nothing is filled from a descriptor).  Shapes,
// offsets and columns come from the one layer table (nlr_obj_layers.h): ObjTrainLin / ObjTrainCls are that table as the
// weight-gradient kernels read it (obj_train_cls), the flat-buffer layouts are its w_off / b_off, the kernel's columns its nlr_obj_cols.
// The workspace, the owner -> scan -> scatter launches and ObjApply are those of nlr_objects.hip (obj_carve, obj_make_lists,
// obj_apply_args).
//
//   forward   owner map -> per-class lists (the kernels of nlr_objects_apply) -> nlr_objtrain_kernel<.., FWD = true>: nlr_objmlp_kernel's
//             layout from the weight image nlr_obj_train_pack made of the flat buffers, every Linear summed in the reference's order
//             (one FMA chain from zero, bias last: obj_begin / obj_end<BIAS_LAST = true>).  The walk through the layers is stated here
//             a second time: against nlr_objmlp_kernel it differs in that switch, in the saved layer inputs and ReLU masks, and in
//             clamping a list entry or an owner outside the batch to an idle lane.  A change to the network is made in both.
//   backward  (1) nlr_objtrain_kernel<.., FWD = false>: one lane per owned sample.  It repeats that forward (same code, same bits), writes
//                 every layer's input to `acts` and every Linear's pre-activation gradient to `gacts` (column-major [column][row]:
//                 a wave stores 256 contiguous bytes per column), and scatters the grid-feature gradient into the class's table
//                 gradient (float atomics, like every grid scatter here).  Rows are numbered class after class: the rows of class c
//                 start at the sum of the counts of the classes before it, so both tensors have N * S rows whatever the classes own.
//                 Its FRAME instance (nlr_obj_train_backward_frame) also writes the cotangents of the sample's box-frame point and
//                 direction, [N * S, 3] each, for track and pose refinement (7c / 7d take them with the owner map as a dense list).
//             (2) nlr_objtrain_wgrad_kernel: dW = gacts_l^T . input_l per Linear as a register-tiled f32 FMA GEMM over the rows.  A
//                 workgroup (class, Linear, slice) walks the 64-row chunks slice, slice + 96, ... of the class, stages the chunk in
//                 LDS, and keeps a [64 outputs x 128 inputs] accumulator tile in its 256 threads' registers; the bias gradient and
//                 the per-track sums of the pre-activation gradient (one owner thread per output, in row order) ride along.  Its
//                 results go to the slice's slab; no atomics.
//             (3) nlr_objtrain_sum_kernel adds the slabs in slice order; nlr_objtrain_params_kernel writes d_params - the weight
//                 columns that multiply the latent code are  sum_t  G_t (x) latent_t  of the per-track sums - and
//                 nlr_objtrain_latents_kernel writes d_latents[t] = sum over those Linears of W_latent^T G_t.  No [K, latent_size]
//                 tensor exists anywhere.
//   The same inputs give the same bits in d_params and d_latents: the lists are in sample order, a chunk belongs to one slice, and
//   every sum has a fixed order.

#include <algorithm>

#define NLR_OBJT_SLICES 96      // slabs per (class, Linear)
#define NLR_OBJT_GS 65          // row stride of the staged gradient chunk (floats): lanes read along a row, stores walk a column
#define NLR_OBJT_XS 132         // row stride of the staged input chunk: 16-byte aligned rows, broadcast ds_read_b128
#define NLR_OBJT_XMAX 128       // input columns a Linear may take from `acts` (4 thread groups x 32 accumulators)
#define NLR_OBJT_MAX_TRACKS 128 // per-track sums of a workgroup: [tracks][64] floats of LDS

struct ObjTrainLin {
    uint32_t w_off, b_off, n_out, n_in;  // in the class's flat parameter buffer: weight [n_out, n_in] row-major, bias [n_out]
    uint32_t outp, img_w, img_b;         // in the LDS image: [n_in][outp] at img_w, bias at img_b
    uint32_t g_col;                      // first column of its pre-activation gradient in gacts
    uint32_t n_blk, blk[3][3];           // input blocks that are columns of acts: (acts column, count, first input column)
    uint32_t lat_n, lat_wcol, lat_off;   // input block that is the track's latent code: count, first input column, offset in the code
    uint32_t gt_off;                     // its per-track sums [n_tracks][n_out] in a slab (behind the n_params floats)
};
struct ObjTrainCls {
    uint32_t n_lin, n_params, slab_floats, aw, gw;
    ObjTrainLin lin[NLR_OBJ_LINEARS];
};
struct ObjTrainPtrs {
    float *p[NLR_OBJ_MAX_CLASSES];
};

// the tables and the latent codes live in the caller's tensors: point the ObjNets at them, in stream order
__global__ void nlr_objtrain_repoint_kernel(ObjNet *nets, uint32_t nc, ObjTrainPtrs tables) {
    if (threadIdx.x < nc) nets[threadIdx.x].gp.table = tables.p[threadIdx.x];
}

// flat parameter buffers -> LDS images (the padding of an image is zero from its creation and is never written)
__global__ void __launch_bounds__(256) nlr_objtrain_pack_kernel(const ObjTrainCls *__restrict__ tcls, const ObjNet *__restrict__ nets,
                                                               ObjTrainPtrs params) {
    const ObjTrainCls &tc = tcls[blockIdx.z];
    if (blockIdx.y >= tc.n_lin) return;
    const ObjTrainLin &L = tc.lin[blockIdx.y];
    const float *src = params.p[blockIdx.z];
    float *img = const_cast<float *>(nets[blockIdx.z].wpack);
    const uint32_t tot = L.n_out * L.n_in;
    for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < tot + L.n_out; e += gridDim.x * 256) {
        if (e < tot) {
            const uint32_t o = e / L.n_in, i = e - o * L.n_in;
            img[L.img_w + i * L.outp + o] = src[L.w_off + e];
        } else {
            img[L.img_b + (e - tot)] = src[L.b_off + (e - tot)];
        }
    }
}

// ---- (1) backward by the data ----------------------------------------------------------------------------------------------
struct ObjTrainB {
    const float *g_density, *g_rgb;  // [N,S], [3,N,S]
    float *acts, *gacts;             // [aw][cap], [gw][cap]
    ObjTrainPtrs grad_tables;
    float *g_pts, *g_dirs;           // [N*S, 3] each, NULL = not wanted: read by the FRAME instance only
};

template <int OUT>
__device__ __forceinline__ float obj_dot_row(const float *wrow, const float (&g)[OUT]) {
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int o = 0; o < OUT; o += 4) {
        const f32x4 w = *reinterpret_cast<const f32x4 *>(wrow + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = fmaf(w[e], g[o + e], s[e]);
    }
    return (s[0] + s[1]) + (s[2] + s[3]);
}

// adjoint of nlr_level_accum_m with w_erf = 1: the 8 corner weights times the level's feature gradient, added into the table gradient
template <int C, int MODE>
__device__ __forceinline__ void obj_level_scatter_m(const GridParams &gp, uint32_t level, const Gauss &g, const float *gf, float *gt) {
    float pos[3];
    uint32_t pg[3];
    nlr_level_cell(gp, level, g, pg, pos);
    if (gp.interp == 1) {
#pragma unroll
        for (int d = 0; d < 3; ++d) pos[d] = pos[d] * pos[d] * (3.0f - 2.0f * pos[d]);
    }
    uint32_t idx[8];
    nlr_corner_idx<MODE>(gp, level, pg, idx);
    float *grid = gt + (size_t)gp.offset[level] * C;
    const float wx[2] = {1 - pos[0], pos[0]}, wy[2] = {1 - pos[1], pos[1]}, wz[2] = {1 - pos[2], pos[2]};
#pragma unroll
    for (int c8 = 0; c8 < 8; ++c8) {
        const float w = (wx[c8 & 1] * wy[(c8 >> 1) & 1]) * wz[(c8 >> 2) & 1];
#pragma unroll
        for (int c = 0; c < C; ++c) atomicAdd(grid + (size_t)idx[c8] * C + c, w * gf[c]);
    }
}
template <int C>
__device__ __forceinline__ void obj_level_scatter(const GridParams &gp, uint32_t level, const Gauss &g, const float *gf, float *gt) {
    const uint32_t mode = gp.mode[level];
    if (mode == 0) obj_level_scatter_m<C, 0>(gp, level, g, gf, gt);
    else if (mode == 1) obj_level_scatter_m<C, 1>(gp, level, g, gf, gt);
    else obj_level_scatter_m<C, 2>(gp, level, g, gf, gt);
}

__device__ __forceinline__ uint32_t obj_pick_mask(const uint32_t (&mv)[NLR_OBJ_MAX_DEPTH], uint32_t i) {
    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < NLR_OBJ_MAX_DEPTH; ++j) m = j == i ? mv[j] : m;
    return m;
}

// the rows of class c: [row0, row0 + count) of acts / gacts, clipped to the capacity whatever the count buffer holds
__device__ __forceinline__ void obj_class_rows(const uint32_t *counts, uint32_t c, uint32_t cap, uint32_t &row0, uint32_t &count) {
    uint64_t r = 0;
    for (uint32_t j = 0; j < c; ++j) r += counts[j];
    count = counts[c];
    if (r >= cap) {
        row0 = 0;
        count = 0;
        return;
    }
    row0 = (uint32_t)r;
    if (count > cap - row0) count = cap - row0;
}

// FWD: the forward alone - results written over a.density / a.rgb / a.sem (rgb NULL: density and semantic only), nothing saved.
// Otherwise the backward: the same forward again (same code, same bits), then the layers walked back.
// FRAME (backward only): also the cotangents of the box frame, row m = ray * S + k of t.g_pts = d loss / d po (the point
// nlr_box_coords returns) and of t.g_dirs = d loss / d de (the direction nlr_box_dir returns); either pointer may be NULL.
//   po enters through the grid alone, g.x = (po + 1) / 2: g_po = 0.5 * sum over the levels of nlr_level_grad on the level's feature
//   gradient (the cell and the smoothstep branch of the forward; zero outside the unit cube).
//   de enters every Linear that takes the concatenated input (view layer 0, view layer skip + 1, rgb_layer when D - 1 == skip) through
//   the columns [de | sin(2^j de) | sin(2^j de + pi/2)].  While the walk has a consumer's pre-activation gradient in hand it adds
//   W[column] . g to that column's gradient (consumers in the order of the walk, columns ascending), and the chain through the
//   sines needs no new transcendental: cos(x) = ds1, cos(x + pi/2) = -ds0.
// Only rows of owned samples are written: the launcher clears both buffers on the stream first.  Everything the plain instance
// computes is computed by the same expressions in the same order.
template <int C, int LMAX, bool FWD, bool FRAME = false>
__global__ void __launch_bounds__(64 * NLR_OBJ_WAVES) nlr_objtrain_kernel(const ObjNet *__restrict__ nets, ObjApply a, ObjTrainB t) {
    const ObjNet &net = nets[blockIdx.y];
    const uint32_t *list = a.lists + (size_t)blockIdx.y * a.cap;
    __shared__ __attribute__((aligned(16))) float wl[NLR_OBJ_WMAX];
    __shared__ float slab_a[NLR_OBJ_WAVES][64 * 64];  // hidden units, bottleneck; then the bottleneck gradient, the hidden gradient
    __shared__ float slab_v[NLR_OBJ_WAVES][32 * 64];  // view layers; then a view layer's input gradient
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t row0, count;
    obj_class_rows(a.counts, blockIdx.y, a.cap, row0, count);
    if (blockIdx.x * (64 * NLR_OBJ_WAVES) >= count) return;  // (the whole workgroup)
    for (uint32_t i = threadIdx.x * 4; i < net.wfloats; i += 64 * NLR_OBJ_WAVES * 4)
        *reinterpret_cast<f32x4 *>(wl + i) = *reinterpret_cast<const f32x4 *>(net.wpack + i);
    __syncthreads();
    float *sa = slab_a[wave], *sv = slab_v[wave];
    const size_t cap = a.cap;
    const ObjCols col = net.cols();  // columns of acts / gacts (nlr_obj_layers.h)
    float *gt = FWD ? nullptr : t.grad_tables.p[blockIdx.y];
    const bool want_rgb = !FWD || a.rgb != nullptr, save = !FWD;
    for (uint32_t base = (blockIdx.x * NLR_OBJ_WAVES + wave) * 64; base < count; base += gridDim.x * (64 * NLR_OBJ_WAVES)) {
        bool valid = base + lane < count;
        uint32_t m = list[valid ? base + lane : count - 1];
        if (m >= a.cap) {  // (a list this plan's forward did not write)
            m = 0;
            valid = false;
        }
        const uint32_t ray = m / a.S, k = m - ray * a.S;
        float pw[3], po[3];
        nlr_interval_midpoint(a.tdist, a.origins, a.dirs, a.S, ray, k, pw);
        uint32_t tr = (uint32_t)a.winner[m];
        if (tr >= a.n_obj) {
            tr = 0;
            valid = false;
        }
        const f32x4 *b = reinterpret_cast<const f32x4 *>(a.box + ((size_t)ray * a.n_obj + tr) * 8);  // (32-byte records of a float array)
        const f32x4 b0 = b[0], b1 = b[1];
        nlr_box_coords(b0, b1, pw, po);
        Gauss g;
        g.x0 = (po[0] + 1.0f) / 2.0f;
        g.x1 = (po[1] + 1.0f) / 2.0f;
        g.x2 = (po[2] + 1.0f) / 2.0f;
        g.zs = 0.0f;
        float de[3], ds0[3 * NLR_OBJ_MAX_DEG], ds1[3 * NLR_OBJ_MAX_DEG];
        if (want_rgb) {
            float vd[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) vd[c] = a.viewdirs[(size_t)ray * 3 + c];
            nlr_box_dir(b0, b1, vd, de);
#pragma unroll
            for (int j = 0; j < NLR_OBJ_MAX_DEG; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float xb = de[c] * (float)(1 << j);
                    ds0[3 * j + c] = sinf(xb);
                    ds1[3 * j + c] = sinf(xb + 0.5f * 3.14159265358979323846f);
                }
        }
        float gf[LMAX * C];
#pragma unroll
        for (int l = 0; l < LMAX; ++l) {
            float acc[C];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = 0.0f;
            if ((uint32_t)l < net.gp.L) nlr_level_accum<float, C>(net.gp, l, g, 1.0f, acc);
#pragma unroll
            for (int c = 0; c < C; ++c) gf[l * C + c] = acc[c];
        }
        float *ar = t.acts + (size_t)row0 + base + lane, *gr = t.gacts + (size_t)row0 + base + lane;  // this lane's row; column stride cap
        if (save && valid) {
#pragma unroll
            for (int j = 0; j < LMAX * C; ++j)
                if ((uint32_t)j < net.n_grid) ar[j * cap] = gf[j];
#pragma unroll
            for (int c = 0; c < 3; ++c) ar[(col.cDE + c) * cap] = de[c];
#pragma unroll
            for (int j = 0; j < 3 * NLR_OBJ_MAX_DEG; ++j)
                if ((uint32_t)j < 3 * net.deg) {
                    ar[(col.cDE + 3 + j) * cap] = ds0[j];
                    ar[(col.cDE + 3 + 3 * net.deg + j) * cap] = ds1[j];
                }
        }
        const float *lat = net.latents + (size_t)tr * net.lat_size;
        // ---- the forward, layer by layer as nlr_objmlp_kernel walks it, every Linear summed as the reference sums it (obj_begin /
        // obj_end<true>); the backward also writes every layer's output to acts
        uint64_t mh = 0;  // hidden unit o passed its ReLU
        {
            float h[64];
            obj_begin<true, 64>(h, wl + net.o_bd0);
            obj_seg_reg<64, LMAX * C>(h, wl + net.o_d0, 0, net.n_grid, gf);
            obj_seg_mem<64>(h, wl + net.o_d0, net.n_grid, net.lat_shape, lat);
            obj_end<true, 64>(h, wl + net.o_bd0);
#pragma unroll
            for (int o = 0; o < 64; ++o) {
                const float r = fmaxf(h[o], 0.0f);
                sa[o * 64 + lane] = r;
                mh |= (uint64_t)(h[o] > 0.0f) << o;
                if (save && valid) ar[(col.cH0 + o) * cap] = r;
            }
        }
        float xd;
        {
            float x0 = 0.0f;  // output 0 of density_layer.2, the raw density
            for (uint32_t kk = 0; kk < 64; ++kk) x0 = fmaf(wl[net.o_d2 + kk * 64], sa[kk * 64 + lane], x0);
            x0 = x0 + wl[net.o_bd2];
            xd = x0 + net.density_bias;
            if (FWD) {
                if (valid) a.density[m] = xd > 20.0f ? xd : log1pf(expf(xd));  // F.softplus, models.py:1116
                if (valid && a.sem) {  // fixed_semantic: one-hot of the class (models.py:1124-1130)
                    for (uint32_t c = 0; c < a.K; ++c) a.sem[(size_t)c * a.N * a.S + m] = ((int32_t)c == net.class_type) ? 1.0f : 0.0f;
                }
                if (!want_rgb) continue;
            }
            float x[64];
            obj_begin<true, 64>(x, wl + net.o_bd2);
            obj_seg_lds<64>(x, wl + net.o_d2, 0, 64, sa, lane);
            obj_end<true, 64>(x, wl + net.o_bd2);
#pragma unroll
            for (int o = 0; o < 64; ++o) {
                sa[o * 64 + lane] = x[o];
                if (save && valid && (uint32_t)o < net.BW) ar[(col.cBOT + o) * cap] = x[o];
            }
        }
        const float *lat_tex = lat + net.lat_tex_off;
        uint32_t mv[NLR_OBJ_MAX_DEPTH] = {0, 0, 0, 0};  // unit o of view layer i passed its ReLU
        for (uint32_t i = 0; i < net.D; ++i) {
            float h[32];
            const float *wv = wl + net.o_v[i];
            obj_begin<true, 32>(h, wl + net.o_bv[i]);
            uint32_t row = 0;
            if (i > 0) {
                obj_seg_lds<32>(h, wv, 0, net.W, sv, lane);
                row = net.W;
            }
            if (i == 0 || i - 1 == net.skip) {
                obj_seg_lds<32>(h, wv, row, net.BW, sa, lane);
                obj_seg_reg<32, 3>(h, wv, row + net.BW, 3, de);
                obj_seg_reg<32, 3 * NLR_OBJ_MAX_DEG>(h, wv, row + net.BW + 3, 3 * net.deg, ds0);
                obj_seg_reg<32, 3 * NLR_OBJ_MAX_DEG>(h, wv, row + net.BW + 3 + 3 * net.deg, 3 * net.deg, ds1);
                obj_seg_mem<32>(h, wv, row + net.BW + net.DE, net.lat_tex, lat_tex);
            }
            obj_end<true, 32>(h, wl + net.o_bv[i]);
            uint32_t mk = 0;
#pragma unroll
            for (int o = 0; o < 32; ++o) {
                const float r = fmaxf(h[o], 0.0f);
                sv[o * 64 + lane] = r;
                mk |= (uint32_t)(h[o] > 0.0f) << o;
                if (save && valid && (uint32_t)o < net.W) ar[(col.cV + i * net.W + o) * cap] = r;
            }
#pragma unroll
            for (uint32_t j = 0; j < NLR_OBJ_MAX_DEPTH; ++j) mv[j] = j == i ? mk : mv[j];
        }
        float c4[4];
        const float *wr = wl + net.o_rgb;
        obj_begin<true, 4>(c4, wl + net.o_brgb);
        obj_seg_lds<4>(c4, wr, 0, net.W, sv, lane);
        if (net.D - 1 == net.skip) {
            obj_seg_lds<4>(c4, wr, net.W, net.BW, sa, lane);
            obj_seg_reg<4, 3>(c4, wr, net.W + net.BW, 3, de);
            obj_seg_reg<4, 3 * NLR_OBJ_MAX_DEG>(c4, wr, net.W + net.BW + 3, 3 * net.deg, ds0);
            obj_seg_reg<4, 3 * NLR_OBJ_MAX_DEG>(c4, wr, net.W + net.BW + 3 + 3 * net.deg, 3 * net.deg, ds1);
            obj_seg_mem<4>(c4, wr, net.W + net.BW + net.DE, net.lat_tex, lat_tex);
        }
        obj_end<true, 4>(c4, wl + net.o_brgb);
        if (FWD) {
            if (valid) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {  // models.py:1251-1255
                    const float sg = 1.0f / (1.0f + expf(-(net.premul * c4[c] + net.rgb_bias)));
                    a.rgb[(size_t)c * a.N * a.S + m] = sg * (1.0f + 2.0f * net.rgb_pad) - net.rgb_pad;
                }
            }
            continue;
        }
        // ---- backward.  rgb = sigmoid(premul * c4 + rgb_bias) * (1 + 2 pad) - pad (models.py:1251-1255)
        float gc[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float sg = 1.0f / (1.0f + expf(-(net.premul * c4[c] + net.rgb_bias)));
            const float up = valid ? t.g_rgb[(size_t)c * a.N * a.S + m] : 0.0f;
            gc[c] = ((up * (1.0f + 2.0f * net.rgb_pad)) * (sg * (1.0f - sg))) * net.premul;
            if (valid) gr[(col.gRGB + c) * cap] = gc[c];
        }
#pragma unroll
        for (int o = 0; o < 64; ++o) sa[o * 64 + lane] = 0.0f;  // the bottleneck gradient collects here (every read of the bottleneck is done)
        float gv[32];  // pre-activation gradient of the view layer in hand
        {
            const uint32_t mk = obj_pick_mask(mv, net.D - 1);
#pragma unroll
            for (int o = 0; o < 32; ++o) {
                const f32x4 w = *reinterpret_cast<const f32x4 *>(wr + ((uint32_t)o < net.W ? o : 0) * 4);
                const float s = (w[0] * gc[0] + w[1] * gc[1]) + w[2] * gc[2];
                gv[o] = ((uint32_t)o < net.W && ((mk >> o) & 1u)) ? s : 0.0f;
            }
            if (net.D - 1 == net.skip)
                for (uint32_t kk = 0; kk < net.BW; ++kk) {
                    const f32x4 w = *reinterpret_cast<const f32x4 *>(wr + (net.W + kk) * 4);
                    sa[kk * 64 + lane] += (w[0] * gc[0] + w[1] * gc[1]) + w[2] * gc[2];
                }
        }
        // FRAME: gradient of the direction encoding's columns, [de | ds0 | ds1]
        float ge_de[3] = {0.0f, 0.0f, 0.0f}, ge_s0[3 * NLR_OBJ_MAX_DEG], ge_s1[3 * NLR_OBJ_MAX_DEG];
#pragma unroll
        for (int j = 0; j < 3 * NLR_OBJ_MAX_DEG; ++j) ge_s0[j] = ge_s1[j] = 0.0f;
        const bool want_dirs = FRAME && t.g_dirs != nullptr;
        if (want_dirs && net.D - 1 == net.skip) {
            const float *we = wr + (net.W + net.BW) * 4;
            auto dot3 = [&](uint32_t q) {
                const f32x4 w = *reinterpret_cast<const f32x4 *>(we + q * 4);
                return (w[0] * gc[0] + w[1] * gc[1]) + w[2] * gc[2];
            };
#pragma unroll
            for (int c = 0; c < 3; ++c) ge_de[c] += dot3(c);
#pragma unroll
            for (int j = 0; j < 3 * NLR_OBJ_MAX_DEG; ++j)
                if ((uint32_t)j < 3 * net.deg) ge_s0[j] += dot3(3 + j);
#pragma unroll
            for (int j = 0; j < 3 * NLR_OBJ_MAX_DEG; ++j)
                if ((uint32_t)j < 3 * net.deg) ge_s1[j] += dot3(3 + 3 * net.deg + j);
        }
        for (uint32_t ii = net.D; ii > 0; --ii) {
            const uint32_t i = ii - 1;
            if (valid) {
#pragma unroll
                for (int o = 0; o < 32; ++o)
                    if ((uint32_t)o < net.W) gr[(col.gV + i * net.W + o) * cap] = gv[o];
            }
            const float *wv = wl + net.o_v[i];
            uint32_t row = 0;
            if (i > 0) {
                for (uint32_t kk = 0; kk < net.W; ++kk) sv[kk * 64 + lane] = obj_dot_row<32>(wv + kk * 32, gv);
                row = net.W;
            }
            if (i == 0 || i - 1 == net.skip)
                for (uint32_t kk = 0; kk < net.BW; ++kk) sa[kk * 64 + lane] += obj_dot_row<32>(wv + (row + kk) * 32, gv);
            if (want_dirs && (i == 0 || i - 1 == net.skip)) {
                const float *we = wv + (row + net.BW) * 32;
#pragma unroll
                for (int c = 0; c < 3; ++c) ge_de[c] += obj_dot_row<32>(we + c * 32, gv);
#pragma unroll
                for (int j = 0; j < 3 * NLR_OBJ_MAX_DEG; ++j)
                    if ((uint32_t)j < 3 * net.deg) ge_s0[j] += obj_dot_row<32>(we + (3 + j) * 32, gv);
#pragma unroll
                for (int j = 0; j < 3 * NLR_OBJ_MAX_DEG; ++j)
                    if ((uint32_t)j < 3 * net.deg) ge_s1[j] += obj_dot_row<32>(we + (3 + 3 * net.deg + j) * 32, gv);
            }
            if (i > 0) {
                const uint32_t mk = obj_pick_mask(mv, i - 1);
#pragma unroll
                for (int o = 0; o < 32; ++o) {
                    const float s = sv[o * 64 + lane];
                    gv[o] = ((uint32_t)o < net.W && ((mk >> o) & 1u)) ? s : 0.0f;
                }
            }
        }
        {
            float gb[64];  // gradient of density_layer.2's output: the view layers' share, and softplus'(raw + bias) on output 0
#pragma unroll
            for (int o = 0; o < 64; ++o) {
                const float s = sa[o * 64 + lane];
                gb[o] = (uint32_t)o < net.BW ? s : 0.0f;
            }
            const float sp = xd > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-xd));
            gb[0] += valid ? t.g_density[m] * sp : 0.0f;
            if (valid) {
#pragma unroll
                for (int o = 0; o < 64; ++o)
                    if ((uint32_t)o < net.BW) gr[(col.gBOT + o) * cap] = gb[o];
            }
            for (uint32_t kk = 0; kk < 64; ++kk) {
                float s = obj_dot_row<64>(wl + net.o_d2 + kk * 64, gb);
                s = ((mh >> kk) & 1ull) ? s : 0.0f;
                sa[kk * 64 + lane] = s;
                if (valid) gr[kk * cap] = s;
            }
        }
        float gh[64];
#pragma unroll
        for (int o = 0; o < 64; ++o) gh[o] = sa[o * 64 + lane];
        float gfe[LMAX * C];
#pragma unroll
        for (int j = 0; j < LMAX * C; ++j) gfe[j] = (uint32_t)j < net.n_grid ? obj_dot_row<64>(wl + net.o_d0 + j * 64, gh) : 0.0f;
        if (valid && gt && !nlr_outside_unit_cube(g)) {
#pragma unroll
            for (int l = 0; l < LMAX; ++l)
                if ((uint32_t)l < net.gp.L) obj_level_scatter<C>(net.gp, l, g, gfe + l * C, gt);
        }
        if (want_dirs && valid) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float s = ge_de[c];
#pragma unroll
                for (int j = 0; j < NLR_OBJ_MAX_DEG; ++j)
                    if ((uint32_t)j < net.deg)
                        s += (float)(1 << j) * (ds1[3 * j + c] * ge_s0[3 * j + c] - ds0[3 * j + c] * ge_s1[3 * j + c]);
                t.g_dirs[(size_t)m * 3 + c] = s;
            }
        }
        if (FRAME && t.g_pts && valid) {
            float gpo[3] = {0.0f, 0.0f, 0.0f};
            if (!nlr_outside_unit_cube(g)) {  // (an owned sample is strictly inside its box; outside the cube the encoding is constant zero)
#pragma unroll
                for (int l = 0; l < LMAX; ++l)
                    if ((uint32_t)l < net.gp.L) {
                        float dp[3], tri;
                        nlr_level_grad<float, C>(net.gp, l, g, gfe + l * C, dp, tri);
#pragma unroll
                        for (int d = 0; d < 3; ++d) gpo[d] += dp[d];
                    }
            }
#pragma unroll
            for (int d = 0; d < 3; ++d) t.g_pts[(size_t)m * 3 + d] = 0.5f * gpo[d];
        }
    }
}

// ---- (2) weight, bias and per-track gradients ---------------------------------------------------------------------------------
struct ObjTrainW {
    const uint32_t *lists, *counts;
    const int32_t *winner;
    uint32_t cap, n_tracks;
    const float *acts, *gacts;
    float *slabs;  // [NLR_OBJT_SLICES][n_classes][slab_stride]
    uint32_t slab_stride;
};

__global__ void __launch_bounds__(256) nlr_objtrain_wgrad_kernel(const ObjTrainCls *__restrict__ tcls, ObjTrainW a) {
    const uint32_t c = blockIdx.z;
    const ObjTrainCls &tc = tcls[c];
    if (blockIdx.y >= tc.n_lin) return;
    const ObjTrainLin &L = tc.lin[blockIdx.y];
    __shared__ float Gs[64 * NLR_OBJT_GS];
    __shared__ __attribute__((aligned(16))) float Xs[64 * NLR_OBJT_XS];
    __shared__ uint32_t trk[64];
    __shared__ float Gt[NLR_OBJT_MAX_TRACKS * 64];
    const uint32_t o = threadIdx.x & 63, q = threadIdx.x >> 6;
    uint32_t row0, count;
    obj_class_rows(a.counts, c, a.cap, row0, count);
    const uint32_t *list = a.lists + (size_t)c * a.cap;
    const size_t cap = a.cap;
    if (L.lat_n)
        for (uint32_t i = threadIdx.x; i < a.n_tracks * 64; i += 256) Gt[i] = 0.0f;
    // this thread's staging columns: input column xi = q, q + 4, .. -> its column of acts (or none)
    float acc[32], accb = 0.0f;
#pragma unroll
    for (int j = 0; j < 32; ++j) acc[j] = 0.0f;
    for (uint32_t chunk = blockIdx.x; (size_t)chunk * 64 < count; chunk += NLR_OBJT_SLICES) {
        const uint32_t r0 = chunk * 64, nrows = count - r0 < 64 ? count - r0 : 64;
        const bool in = o < nrows;  // (staging: o is the row)
        __syncthreads();            // the previous chunk has been read
        const float *gsrc = a.gacts + (size_t)row0 + r0 + o, *xsrc = a.acts + (size_t)row0 + r0 + o;
        for (uint32_t col = q; col < 64; col += 4) Gs[o * NLR_OBJT_GS + col] = (in && col < L.n_out) ? gsrc[(L.g_col + col) * cap] : 0.0f;
        for (uint32_t xi = q; xi < NLR_OBJT_XMAX; xi += 4) {
            uint32_t rest = xi, col = 0xffffffffu;
            for (uint32_t bk = 0; bk < L.n_blk; ++bk) {
                if (rest < L.blk[bk][1]) {
                    col = L.blk[bk][0] + rest;
                    break;
                }
                rest -= L.blk[bk][1];
            }
            Xs[o * NLR_OBJT_XS + xi] = (in && col != 0xffffffffu) ? xsrc[col * cap] : 0.0f;
        }
        if (L.lat_n && threadIdx.x < 64) {
            uint32_t tr = 0;
            if (in) {
                const uint32_t m = list[r0 + o];
                tr = m < a.cap ? (uint32_t)a.winner[m] : 0;
                tr = tr < a.n_tracks ? tr : 0;
            }
            trk[o] = tr;
        }
        __syncthreads();
        for (uint32_t r = 0; r < nrows; ++r) {
            const float gg = Gs[r * NLR_OBJT_GS + o];
            const float *xr = Xs + r * NLR_OBJT_XS + q * 32;
#pragma unroll
            for (int j = 0; j < 32; j += 4) {
                const f32x4 x = *reinterpret_cast<const f32x4 *>(xr + j);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j + e] = fmaf(gg, x[e], acc[j + e]);
            }
            if (q == 0) {
                accb += gg;
                if (L.lat_n) Gt[trk[r] * 64 + o] += gg;  // (one thread owns output o: row order)
            }
        }
    }
    // the slice's slab: weights at their place in the flat buffer (the latent columns are not written here), bias, per-track sums
    float *slab = a.slabs + ((size_t)blockIdx.x * gridDim.z + c) * a.slab_stride;
    if (o < L.n_out) {
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            uint32_t rest = q * 32 + j;
            for (uint32_t bk = 0; bk < L.n_blk; ++bk) {
                if (rest < L.blk[bk][1]) {
                    slab[L.w_off + o * L.n_in + L.blk[bk][2] + rest] = acc[j];
                    break;
                }
                rest -= L.blk[bk][1];
            }
        }
        if (q == 0) slab[L.b_off + o] = accb;
    }
    if (L.lat_n) {
        // the weight columns that multiply the latent code come from the per-track sums (nlr_objtrain_params_kernel): zeros here, so that
        // every float of a slab is written
        for (uint32_t i = threadIdx.x; i < L.n_out * L.lat_n; i += 256) {
            const uint32_t oo = i / L.lat_n, kk = i - oo * L.lat_n;
            slab[L.w_off + oo * L.n_in + L.lat_wcol + kk] = 0.0f;
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < a.n_tracks * 64; i += 256) {
            const uint32_t tk = i >> 6, oo = i & 63;
            if (oo < L.n_out) slab[L.gt_off + tk * L.n_out + oo] = Gt[i];
        }
    }
}

// ---- (3) slabs -> totals -> d_params, d_latents ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) nlr_objtrain_sum_kernel(const ObjTrainCls *__restrict__ tcls, const float *__restrict__ slabs,
                                                              uint32_t slab_stride, float *__restrict__ totals) {
    const uint32_t c = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= tcls[c].slab_floats) return;
    float s = 0.0f;
    for (uint32_t sl = 0; sl < NLR_OBJT_SLICES; ++sl) s += slabs[((size_t)sl * gridDim.y + c) * slab_stride + j];
    totals[(size_t)c * slab_stride + j] = s;
}

__global__ void __launch_bounds__(256) nlr_objtrain_params_kernel(const ObjTrainCls *__restrict__ tcls, const float *__restrict__ totals,
                                                                 uint32_t slab_stride, const float *__restrict__ latents, uint32_t lat_size,
                                                                 uint32_t n_tracks, ObjTrainPtrs d_params) {
    const uint32_t c = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const ObjTrainCls &tc = tcls[c];
    if (j >= tc.n_params) return;
    const float *tot = totals + (size_t)c * slab_stride;
    float v = tot[j];
    for (uint32_t li = 0; li < tc.n_lin; ++li) {
        const ObjTrainLin &L = tc.lin[li];
        if (!L.lat_n || j < L.w_off || j >= L.w_off + L.n_out * L.n_in) continue;
        const uint32_t o = (j - L.w_off) / L.n_in, i = (j - L.w_off) - o * L.n_in;
        if (i < L.lat_wcol || i >= L.lat_wcol + L.lat_n) continue;
        v = 0.0f;  // a weight on the latent code: sum over the tracks of (sum of its output's gradient over the track) * code
        for (uint32_t tk = 0; tk < n_tracks; ++tk)
            v = fmaf(tot[L.gt_off + tk * L.n_out + o], latents[(size_t)tk * lat_size + L.lat_off + (i - L.lat_wcol)], v);
    }
    d_params.p[c][j] = v;
}

__global__ void __launch_bounds__(256) nlr_objtrain_latents_kernel(const ObjTrainCls *__restrict__ tcls, const ObjNet *__restrict__ nets,
                                                                  const int32_t *__restrict__ track_class, const float *__restrict__ totals,
                                                                  uint32_t slab_stride, uint32_t lat_size, uint32_t n_tracks,
                                                                  float *__restrict__ d_latents) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_tracks * lat_size) return;
    const uint32_t tk = e / lat_size, kk = e - tk * lat_size;
    const uint32_t c = (uint32_t)track_class[tk];
    const ObjTrainCls &tc = tcls[c];
    const float *tot = totals + (size_t)c * slab_stride, *img = nets[c].wpack;
    float s = 0.0f;
    for (uint32_t li = 0; li < tc.n_lin; ++li) {
        const ObjTrainLin &L = tc.lin[li];
        if (kk < L.lat_off || kk >= L.lat_off + L.lat_n) continue;
        const float *wrow = img + L.img_w + (size_t)(L.lat_wcol + (kk - L.lat_off)) * L.outp;  // the image holds W transposed
        for (uint32_t o = 0; o < L.n_out; ++o) s = fmaf(wrow[o], tot[L.gt_off + tk * L.n_out + o], s);
    }
    d_latents[e] = s;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct NlrObjTrainPlan {
    NlrObjects *objs = nullptr;  // the ObjNets, their images, the latent table and track_class: what nlr_objects_apply_impl runs on
    std::vector<ObjTrainCls> cls;
    ObjTrainCls *cls_dev = nullptr;
    float *lat_dev = nullptr;    // objs' latent table [n_tracks, lat_size]: the caller's codes are copied here on the stream
    uint32_t lat_size = 0, slab_stride = 0, aw = 0, gw = 0;
    ~NlrObjTrainPlan() {
        if (cls_dev) (void)hipFree(cls_dev);
        delete objs;
    }
};

// host arithmetic only: the offsets (weight, bias per Linear) of class `cls` of a descriptor, then the buffer's length; returns the
// number of entries written (2 per Linear + 1)
extern "C" int nlr_obj_train_desc_layout(const NlrObjectsDesc *d, uint32_t cls, uint32_t *offsets_host, uint32_t capacity) {
    NLR_CHECK_ARG(d && d->classes && offsets_host && cls < d->n_classes, "obj_train_desc_layout: NULL argument or class %u outside the descriptor", cls);
    ObjLayers t;
    char msg[256];
    if (!nlr_obj_layers(d->classes[cls], "obj_train_desc_layout", cls, t, msg, sizeof(msg))) NLR_FAIL(NLR_ERR_UNSUPPORTED, "%s", msg);
    NLR_CHECK_ARG(capacity >= 2 * t.n_lin + 1, "obj_train_desc_layout: buffer too small (%u entries)", 2 * t.n_lin + 1);
    for (uint32_t i = 0; i < t.n_lin; ++i) offsets_host[2 * i] = t.lin[i].w_off, offsets_host[2 * i + 1] = t.lin[i].b_off;
    offsets_host[2 * t.n_lin] = t.n_params;
    return (int)(2 * t.n_lin + 1);
}

// the layer table as the weight-gradient kernels read it: acts blocks and the latent block apart, the per-track sums behind the parameters
static ObjTrainCls obj_train_cls(const ObjLayers &t, uint32_t n_tracks) {
    ObjTrainCls tc;
    memset(&tc, 0, sizeof(tc));
    tc.n_lin = t.n_lin, tc.n_params = t.n_params, tc.aw = t.col.aw, tc.gw = t.col.gw;
    tc.slab_floats = t.n_params;
    for (uint32_t i = 0; i < t.n_lin; ++i) {
        const ObjLinear &s = t.lin[i];
        ObjTrainLin &L = tc.lin[i];
        L.w_off = s.w_off, L.b_off = s.b_off, L.n_out = s.n_out, L.n_in = s.n_in;
        L.outp = s.outp, L.img_w = s.img_w, L.img_b = s.img_b, L.g_col = s.g_col;
        L.gt_off = t.n_params;  // (unused where lat_n = 0)
        for (uint32_t k = 0; k < s.n_inputs; ++k) {
            const ObjInput &in = s.in[k];
            if (in.latent()) {  // (a Linear takes at most one half of the code)
                L.lat_n = in.n, L.lat_wcol = in.wcol, L.lat_off = in.src;
                L.gt_off = tc.slab_floats;
                tc.slab_floats += n_tracks * s.n_out;
            } else {
                L.blk[L.n_blk][0] = in.src, L.blk[L.n_blk][1] = in.n, L.blk[L.n_blk][2] = in.wcol;
                ++L.n_blk;
            }
        }
    }
    return tc;
}

// The plan is made of shapes: the object set is laid out and allocated (obj_layout: envelope, table, zeroed images and codes), and
// nlr_obj_train_pack fills the images from the flat buffers.
extern "C" int nlr_obj_train_plan_create(const NlrObjectsDesc *d, NlrObjTrainPlan **out, uint32_t *n_params_host, void *stream) {
    NLR_CHECK_ARG(d && out && n_params_host, "obj_train_plan_create: NULL argument");
    if (d->n_tracks > NLR_OBJT_MAX_TRACKS)
        NLR_FAIL(NLR_ERR_UNSUPPORTED, "obj_train_plan_create: n_tracks = %u, the weight-gradient kernel keeps per-track sums for at most %d",
                 d->n_tracks, NLR_OBJT_MAX_TRACKS);
    for (uint32_t c = 0; d->classes && c < d->n_classes && c < NLR_OBJ_MAX_CLASSES; ++c)
        if (d->classes[c].mlp.grid.table_dtype != 0)
            NLR_FAIL(NLR_ERR_UNSUPPORTED, "obj_train_plan_create: the table gradient is f32, table_dtype must be 0");
    std::unique_ptr<NlrObjects> objs;
    int rc = obj_layout(d, "obj_train_plan_create", objs, (hipStream_t)stream);
    if (rc) return rc;
    std::unique_ptr<NlrObjTrainPlan> p(new NlrObjTrainPlan());
    p->objs = objs.release();
    p->lat_size = d->classes[0].latent_size;
    p->lat_dev = const_cast<float *>(p->objs->cls[0].latents);
    for (uint32_t c = 0; c < d->n_classes; ++c) {
        p->cls.push_back(obj_train_cls(p->objs->layers[c], d->n_tracks));
        const ObjTrainCls &tc = p->cls.back();
        n_params_host[c] = tc.n_params;
        p->slab_stride = std::max(p->slab_stride, (tc.slab_floats + 63u) & ~63u);
        p->aw = std::max(p->aw, tc.aw);
        p->gw = std::max(p->gw, tc.gw);
    }
    NLR_HIP(hipMalloc((void **)&p->cls_dev, p->cls.size() * sizeof(ObjTrainCls)));
    NLR_HIP(hipMemcpyAsync(p->cls_dev, p->cls.data(), p->cls.size() * sizeof(ObjTrainCls), hipMemcpyHostToDevice, (hipStream_t)stream));
    NLR_HIP(hipStreamSynchronize((hipStream_t)stream));
    *out = p.release();
    return NLR_OK;
}

extern "C" void nlr_obj_train_plan_destroy(NlrObjTrainPlan *p) { delete p; }

// offsets (weight, bias) of every Linear of class `cls` in its flat buffer, in the order density_layer.0, density_layer.2,
// lin_second_stage_0..D-1, rgb_layer; returns the number of entries
extern "C" int nlr_obj_train_param_layout(const NlrObjTrainPlan *p, uint32_t cls, uint32_t *offsets_host, uint32_t capacity) {
    NLR_CHECK_ARG(p && offsets_host && cls < p->cls.size(), "obj_train_param_layout: NULL argument or class %u outside the plan", cls);
    const ObjTrainCls &tc = p->cls[cls];
    NLR_CHECK_ARG(capacity >= 2 * tc.n_lin, "obj_train_param_layout: buffer too small (%u entries)", 2 * tc.n_lin);
    for (uint32_t i = 0; i < tc.n_lin; ++i) offsets_host[2 * i] = tc.lin[i].w_off, offsets_host[2 * i + 1] = tc.lin[i].b_off;
    return (int)(2 * tc.n_lin);
}

extern "C" int nlr_obj_train_pack(NlrObjTrainPlan *p, const float *const *params, void *stream) {
    NLR_CHECK_ARG(p && params, "obj_train_pack: NULL argument");
    ObjTrainPtrs pp;
    memset(&pp, 0, sizeof(pp));
    for (size_t c = 0; c < p->cls.size(); ++c) {
        NLR_CHECK_ARG(params[c], "obj_train_pack: params[%zu] is NULL", c);
        pp.p[c] = const_cast<float *>(params[c]);
    }
    hipLaunchKernelGGL(nlr_objtrain_pack_kernel, dim3(8, NLR_OBJ_LINEARS, (unsigned)p->cls.size()), dim3(256), 0, (hipStream_t)stream, p->cls_dev,
                       p->objs->nets_dev, pp);
    NLR_LAUNCH_CHECK("nlr_objtrain_pack_kernel");
    return NLR_OK;
}

// the workspace of nlr_objects_apply and, for the backward, acts / gacts / slabs / totals behind it (obj_carve, nlr_objects.hip)
static ObjWorkspace obj_train_carve(const NlrObjTrainPlan *p, void *workspace, uint32_t N, uint32_t S, int backward) {
    const size_t nc = p->cls.size();
    if (!backward) return obj_carve(workspace, nc, N, S, 0, 0, 0, 0);
    return obj_carve(workspace, nc, N, S, p->aw, p->gw, (size_t)NLR_OBJT_SLICES * nc * p->slab_stride, nc * p->slab_stride);
}
extern "C" size_t nlr_obj_train_workspace_bytes(const NlrObjTrainPlan *p, uint32_t N, uint32_t S, int backward) {
    return p ? obj_train_carve(p, nullptr, N, S, backward).bytes : 0;
}

// the checks both passes share; *run = 0: nothing to do
static int obj_train_check(const char *fn, const NlrObjTrainPlan *p, const float *const *tables, const float *latents, const NlrRays *rays,
                           const float *tdist, const float *box_params, uint32_t N, uint32_t S, uint32_t n_obj, const void *workspace,
                           size_t workspace_bytes, int backward, int *run) {
    *run = 0;
    NLR_CHECK_ARG(p, "%s: plan is NULL", fn);
    if (N == 0 || S == 0 || n_obj == 0) return NLR_OK;
    NLR_CHECK_ARG(tables, "%s: tables is NULL", fn);
    for (size_t c = 0; c < p->cls.size(); ++c) NLR_CHECK_ARG(tables[c], "%s: tables[%zu] is NULL", fn, c);
    NLR_CHECK_ARG(latents || p->lat_size == 0, "%s: latents is NULL", fn);
    NLR_CHECK_ARG(rays && rays->origins && rays->directions && rays->viewdirs, "%s: rays (origins / directions / viewdirs) is NULL", fn);
    NLR_CHECK_ARG(tdist, "%s: tdist is NULL", fn);
    NLR_CHECK_ARG(box_params, "%s: box_params is NULL", fn);
    NLR_CHECK_ARG(((uintptr_t)box_params & 15) == 0, "%s: box_params must be 16-byte aligned", fn);
    NLR_CHECK_ARG(n_obj == p->objs->n_tracks, "%s: n_obj = %u boxes per ray, the plan has %u tracks", fn, n_obj, p->objs->n_tracks);
    NLR_CHECK_ARG((size_t)N * S < (1ull << 32), "%s: N * S = %zu does not fit the 32-bit sample index", fn, (size_t)N * S);
    const size_t need = nlr_obj_train_workspace_bytes(p, N, S, backward);
    if (!workspace || workspace_bytes < need)
        NLR_FAIL(NLR_ERR_WORKSPACE, "%s: workspace %zu B < nlr_obj_train_workspace_bytes() = %zu B", fn, workspace_bytes, need);
    *run = 1;
    return NLR_OK;
}

static int obj_train_bind(NlrObjTrainPlan *p, const float *const *tables, const float *latents, hipStream_t st) {
    ObjTrainPtrs tp;
    memset(&tp, 0, sizeof(tp));
    for (size_t c = 0; c < p->cls.size(); ++c) tp.p[c] = const_cast<float *>(tables[c]);
    hipLaunchKernelGGL(nlr_objtrain_repoint_kernel, dim3(1), dim3(64), 0, st, p->objs->nets_dev, (uint32_t)p->cls.size(), tp);
    NLR_LAUNCH_CHECK("nlr_objtrain_repoint_kernel");
    if (p->lat_size)
        NLR_HIP(hipMemcpyAsync(p->lat_dev, latents, (size_t)p->objs->n_tracks * p->lat_size * 4, hipMemcpyDeviceToDevice, st));
    return NLR_OK;
}

// the backward with tb.g_pts or tb.g_dirs set takes the FRAME instance, everything else the plain ones
static int obj_train_launch(const NlrObjTrainPlan *p, bool fwd, uint32_t N, uint32_t S, const ObjApply &a, const ObjTrainB &tb, hipStream_t st) {
    const NlrObjects *o = p->objs;
    const uint32_t C = o->cls[0].gp.C;
    const bool frame = !fwd && (tb.g_pts || tb.g_dirs);
#define OBJT_LAUNCH(C_, LM)                                                                                                                      \
    if (fwd) hipLaunchKernelGGL((nlr_objtrain_kernel<C_, LM, true>), obj_net_grid(o, N, S), dim3(64 * NLR_OBJ_WAVES), 0, st, o->nets_dev, a, tb); \
    else if (frame)                                                                                                                              \
        hipLaunchKernelGGL((nlr_objtrain_kernel<C_, LM, false, true>), obj_net_grid(o, N, S), dim3(64 * NLR_OBJ_WAVES), 0, st, o->nets_dev, a, tb); \
    else hipLaunchKernelGGL((nlr_objtrain_kernel<C_, LM, false>), obj_net_grid(o, N, S), dim3(64 * NLR_OBJ_WAVES), 0, st, o->nets_dev, a, tb)
    if (C == 2) { OBJT_LAUNCH(2, 8); }
    else if (C == 4) { OBJT_LAUNCH(4, 4); }
    else { OBJT_LAUNCH(1, 16); }
#undef OBJT_LAUNCH
    NLR_LAUNCH_CHECK(fwd ? "nlr_objtrain_kernel (forward)" : "nlr_objtrain_kernel (backward)");
    return NLR_OK;
}

extern "C" int nlr_obj_train_forward(NlrObjTrainPlan *p, const float *const *tables, const float *latents, const NlrRays *rays,
                                     const float *tdist, const float *box_params, uint32_t N, uint32_t S, uint32_t n_obj, float *density,
                                     float *rgb, float *semantic, uint32_t K, int32_t *winner, void *workspace, size_t workspace_bytes,
                                     void *stream) {
    int run = 0, rc = obj_train_check("obj_train_forward", p, tables, latents, rays, tdist, box_params, N, S, n_obj, workspace, workspace_bytes, 0, &run);
    if (rc || !run) return rc;
    NLR_CHECK_ARG(density, "obj_train_forward: density is NULL");
    NLR_CHECK_ARG(winner, "obj_train_forward: winner is NULL");
    hipStream_t st = (hipStream_t)stream;
    if ((rc = obj_train_bind(p, tables, latents, st))) return rc;
    // owner map and lists as nlr_objects_apply_impl makes them (same function, same carving), then this file's forward
    const ObjWorkspace w = obj_train_carve(p, workspace, N, S, 0);
    if ((rc = obj_make_lists(p->objs, w, rays, tdist, box_params, N, S, n_obj, winner, st))) return rc;
    ObjTrainB tb;
    memset(&tb, 0, sizeof(tb));
    return obj_train_launch(p, true, N, S, obj_apply_args(w, rays, tdist, box_params, N, S, n_obj, density, rgb, semantic, K), tb, st);
}

// the backward of both entry points; g_pts / g_dirs NULL: not wanted (both NULL: the plain instance of the kernel)
static int obj_train_backward_impl(const char *fn, NlrObjTrainPlan *p, const float *const *tables, const float *latents, const NlrRays *rays,
                                   const float *tdist, const float *box_params, uint32_t N, uint32_t S, uint32_t n_obj, const float *g_density,
                                   const float *g_rgb, float *const *d_params, float *d_latents, float *const *grad_tables, float *g_pts,
                                   float *g_dirs, void *workspace, size_t workspace_bytes, void *stream) {
    int run = 0, rc = obj_train_check(fn, p, tables, latents, rays, tdist, box_params, N, S, n_obj, workspace, workspace_bytes, 1, &run);
    if (rc || !run) return rc;
    NLR_CHECK_ARG(g_density && g_rgb, "%s: g_density / g_rgb is NULL", fn);
    NLR_CHECK_ARG(d_params && grad_tables, "%s: d_params / grad_tables is NULL", fn);
    NLR_CHECK_ARG(d_latents || p->lat_size == 0, "%s: d_latents is NULL", fn);
    const uint32_t nc = (uint32_t)p->cls.size();
    ObjTrainB tb;
    ObjTrainPtrs dp;
    memset(&dp, 0, sizeof(dp));
    memset(&tb, 0, sizeof(tb));
    for (uint32_t c = 0; c < nc; ++c) {
        NLR_CHECK_ARG(d_params[c] && grad_tables[c], "%s: d_params[%u] / grad_tables[%u] is NULL", fn, c, c);
        dp.p[c] = d_params[c];
        tb.grad_tables.p[c] = grad_tables[c];
    }
    hipStream_t st = (hipStream_t)stream;
    if ((rc = obj_train_bind(p, tables, latents, st))) return rc;
    // counts, owner map and lists are the forward's, where it left them in this workspace
    const ObjWorkspace w = obj_train_carve(p, workspace, N, S, 1);
    tb.g_density = g_density, tb.g_rgb = g_rgb, tb.acts = w.acts, tb.gacts = w.gacts;
    tb.g_pts = g_pts, tb.g_dirs = g_dirs;
    // the kernel writes the rows of owned samples only: every other row is the zero of this clear
    for (float *g : {g_pts, g_dirs})
        if (g) NLR_HIP(hipMemsetAsync(g, 0, (size_t)N * S * 3 * sizeof(float), st));
    if ((rc = obj_train_launch(p, false, N, S, obj_apply_args(w, rays, tdist, box_params, N, S, n_obj, nullptr, nullptr, nullptr, 0), tb, st)))
        return rc;
    const ObjTrainW tw = {w.lists, w.counts, w.winner, /*cap*/ N * S, /*n_tracks*/ n_obj, w.acts, w.gacts, w.slabs, p->slab_stride};
    hipLaunchKernelGGL(nlr_objtrain_wgrad_kernel, dim3(NLR_OBJT_SLICES, NLR_OBJ_LINEARS, nc), dim3(256), 0, st, p->cls_dev, tw);
    NLR_LAUNCH_CHECK("nlr_objtrain_wgrad_kernel");
    hipLaunchKernelGGL(nlr_objtrain_sum_kernel, dim3((p->slab_stride + 255) / 256, nc), dim3(256), 0, st, p->cls_dev, w.slabs, p->slab_stride, w.totals);
    NLR_LAUNCH_CHECK("nlr_objtrain_sum_kernel");
    hipLaunchKernelGGL(nlr_objtrain_params_kernel, dim3((p->slab_stride + 255) / 256, nc), dim3(256), 0, st, p->cls_dev, w.totals, p->slab_stride,
                       p->lat_dev, p->lat_size, n_obj, dp);
    NLR_LAUNCH_CHECK("nlr_objtrain_params_kernel");
    if (p->lat_size) {
        hipLaunchKernelGGL(nlr_objtrain_latents_kernel, dim3((n_obj * p->lat_size + 255) / 256), dim3(256), 0, st, p->cls_dev, p->objs->nets_dev,
                           p->objs->track_class, w.totals, p->slab_stride, p->lat_size, n_obj, d_latents);
        NLR_LAUNCH_CHECK("nlr_objtrain_latents_kernel");
    }
    return NLR_OK;
}

extern "C" int nlr_obj_train_backward(NlrObjTrainPlan *p, const float *const *tables, const float *latents, const NlrRays *rays,
                                      const float *tdist, const float *box_params, uint32_t N, uint32_t S, uint32_t n_obj,
                                      const float *g_density, const float *g_rgb, float *const *d_params, float *d_latents,
                                      float *const *grad_tables, void *workspace, size_t workspace_bytes, void *stream) {
    return obj_train_backward_impl("obj_train_backward", p, tables, latents, rays, tdist, box_params, N, S, n_obj, g_density, g_rgb, d_params,
                                   d_latents, grad_tables, nullptr, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int nlr_obj_train_backward_frame(NlrObjTrainPlan *p, const float *const *tables, const float *latents, const NlrRays *rays,
                                            const float *tdist, const float *box_params, uint32_t N, uint32_t S, uint32_t n_obj,
                                            const float *g_density, const float *g_rgb, float *const *d_params, float *d_latents,
                                            float *const *grad_tables, float *g_pts, float *g_dirs, void *workspace, size_t workspace_bytes,
                                            void *stream) {
    return obj_train_backward_impl("obj_train_backward_frame", p, tables, latents, rays, tdist, box_params, N, S, n_obj, g_density, g_rgb,
                                   d_params, d_latents, grad_tables, g_pts, g_dirs, workspace, workspace_bytes, stream);
}
