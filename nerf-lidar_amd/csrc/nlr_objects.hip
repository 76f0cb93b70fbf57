// Dynamic-object branch (scope row f-1, header section 7b): pose blend -> owner of every sample + per-class compaction ->
// object networks, and the adjoints of the box-frame map: by the track (track refinement) and by the ray (pose refinement).  All of
// it on the device.
//
//   ZI/models.py:401-477 loops over tracks and lets every later track overwrite the samples of earlier ones, so a sample
//   belongs to the LAST track whose box contains its interval midpoint.  ZI/obj_utils.py:203-216 (box_pts) decides "inside"
//   by |p_o| < 1 on all three axes of p_o = scale * (R(p_w) + t_w_o), R = rotate_yaw_z with the reference's quirk
//   (y' from the already rotated x', obj_utils.py:106-107).
// The order of the float operations in that map decides on which side of a box face a sample lands, so the map is written
// ONCE, in the nlr_box_* / nlr_track_* device functions below, and every kernel of this file goes through them: the
// per-(ray, track) constants (nlr_track_box_kernel), the owner map (nlr_box_owner_kernel, one thread per sample with the
// track loop in registers: the reference materialises [N, S, N_obj, 3] tensors for this), the networks' inputs
// (nlr_objmlp_kernel) and the forward half of the adjoint (nlr_obj_frame_bwd_kernel).  Built with -ffp-contract=off: the
// multiply / add chains below are the reference's torch expressions, operation by operation.
//   The network of a class is stated as data ONCE, in nlr_obj_layers.h (nlr_obj_layers: the Linears, their input blocks, their places
// in the LDS image, in the flat training buffer and in acts / gacts, the envelope and its messages): the ObjNet offsets here, the
// training plan's layouts and the weight-gradient records of nlr_objects_train.h are made of that table.  An object set is made in two
// steps, obj_layout ("lay out and allocate": the training plan stops there) and obj_fill_images (from NlrLinears).  The launch
// preparation - the carved workspace (obj_carve), owner -> scan -> scatter (obj_make_lists), ObjApply (obj_apply_args), the grid
// (obj_net_grid) - is written once for nlr_objects_apply and the two training entry points.  The walk through the layers is written
// twice, in nlr_objmlp_kernel below and in nlr_objtrain_kernel: they share the segment helpers and the accumulator policy
// (obj_begin / obj_end<BIAS_LAST>, the one numerical difference between them).
#include "nlr_kernels.h"
#include "nlr_grid_level.h"
#include "nlr_objects.h"

#include <memory>
#include <vector>

// ---- the box-frame map ---------------------------------------------------------------------------------------------------
// A box record is the 8 floats nlr_track_box_kernel writes per (ray, track), passed by value as two f32x4:
//   b0 = (cos, sin, t_w_o.x, t_w_o.y), b1 = (t_w_o.z, scale.x, scale.y, scale.z).

// world position of the midpoint of interval k of `ray`
__device__ __forceinline__ void nlr_interval_midpoint(const float *__restrict__ tdist, const float *__restrict__ origins,
                                                      const float *__restrict__ dirs, uint32_t S, uint32_t ray, uint32_t k, float (&p)[3]) {
    const float t0 = tdist[(size_t)ray * (S + 1) + k], t1 = tdist[(size_t)ray * (S + 1) + k + 1];
    const float tm = 0.5f * (t0 + t1);
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = tm * dirs[(size_t)ray * 3 + c] + origins[(size_t)ray * 3 + c];
}

// rotate_yaw_z on (x, y) with the reference's quirk: (sic) y' from the already rotated x' (obj_utils.py:106-107)
__device__ __forceinline__ void nlr_rotate_yaw(float cs, float sn, float x, float y, float &rx, float &ry) {
    rx = cs * x - sn * y;
    ry = sn * rx + cs * y;
}

// world point -> box coordinates (world2object, obj_utils.py:158-170)
__device__ __forceinline__ void nlr_box_coords(f32x4 b0, f32x4 b1, const float (&p)[3], float (&x)[3]) {
    float rx, ry;
    nlr_rotate_yaw(b0[0], b0[1], p[0], p[1], rx, ry);
    x[0] = b1[1] * (rx + b0[2]);
    x[1] = b1[2] * (ry + b0[3]);
    x[2] = b1[3] * (p[2] + b1[0]);
}

// view direction -> normalised box-frame direction (obj_utils.py:171-176)
__device__ __forceinline__ void nlr_box_dir(f32x4 b0, f32x4 b1, const float (&v)[3], float (&d)[3]) {
    float vx, vy;
    nlr_rotate_yaw(b0[0], b0[1], v[0], v[1], vx, vy);
    d[0] = b1[1] * vx;
    d[1] = b1[2] * vy;
    d[2] = b1[3] * v[2];
    const float nrm = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = d[c] / nrm;
}

// box_pts' intersection map (obj_utils.py:203-216): strictly inside on all three axes; branch-free
__device__ __forceinline__ int nlr_box_inside(const float (&x)[3]) {
    return (int)(fabsf(x[0]) < 1.0f) & (int)(fabsf(x[1]) < 1.0f) & (int)(fabsf(x[2]) < 1.0f);
}

// ---- get_pose + world2object constants (obj_utils.py:431-475, :5-28,:158-170) ---------------------------------------------
// The two records of one track closest in time to `time` (torch.sort(time_diff)[..., :2]; on equal distances the earlier record
// first) and the weight of the first.  nlr_track_box_kernel and its adjoint nlr_obj_frame_bwd_kernel both choose through this
// function, so a tie between records cannot fall differently in the two.
__device__ __forceinline__ void nlr_track_records(const float *__restrict__ tr, uint32_t T, float time, uint32_t &i1, uint32_t &i2,
                                                  float &w1) {
    i1 = 0;
    i2 = 0;
    float d1 = INFINITY, d2 = INFINITY;
    for (uint32_t k = 0; k < T; ++k) {
        const float d = fabsf(time - tr[k * 9 + 7]);
        if (d < d1) {
            d2 = d1;
            i2 = i1;
            d1 = d;
            i1 = k;
        } else if (d < d2) {
            d2 = d;
            i2 = k;
        }
    }
    const float t1 = tr[i1 * 9 + 7], t2 = tr[i2 * 9 + 7];
    w1 = fabsf(time - t2) / (fabsf(t1 - t2) + 1e-9f);
    w1 = fminf(fmaxf(w1, 0.0f), 1.0f);
}

// One track at one time: the two records and the weight of the first (nlr_track_records), the blended pose (center3, theta,
// wlh3) and the box record b0 / b1 made of it.  The forward and the forward half of the adjoint.
struct TrackBox {
    uint32_t i1, i2;
    float w1, pose[7];
    f32x4 b0, b1;
};
__device__ __forceinline__ TrackBox nlr_track_box(const float *__restrict__ tr, uint32_t T, float time) {
    TrackBox t;
    nlr_track_records(tr, T, time, t.i1, t.i2, t.w1);
#pragma unroll
    for (int c = 0; c < 7; ++c) t.pose[c] = t.w1 * tr[t.i1 * 9 + c] + (1.0f - t.w1) * tr[t.i2 * 9 + c];
    const float cs = cosf(t.pose[3]), sn = sinf(t.pose[3]);
    float tx, ty;
    nlr_rotate_yaw(cs, sn, -t.pose[0], -t.pose[1], tx, ty);  // t_w_o = rotate_yaw_z(-center, theta)
    t.b0 = f32x4{cs, sn, tx, ty};
    t.b1[0] = -t.pose[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) t.b1[1 + c] = 1.0f / (t.pose[4 + c] / 2.0f + 1e-9f);
    return t;
}

// one thread per (ray, track)
__global__ void __launch_bounds__(256) nlr_track_box_kernel(const float *__restrict__ tracks, const float *__restrict__ ts, uint32_t N,
                                                           uint32_t n_obj, uint32_t T, float *__restrict__ box) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)N * n_obj) return;
    const uint32_t ray = (uint32_t)(i / n_obj), o = (uint32_t)(i - (size_t)ray * n_obj);
    const TrackBox t = nlr_track_box(tracks + (size_t)o * T * 9, T, ts[ray]);
    float *b = box + i * 8;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        b[c] = t.b0[c];
        b[4 + c] = t.b1[c];
    }
}

extern "C" int nlr_track_box_params(const float *tracks, const float *timestamps, uint32_t N, uint32_t n_obj, uint32_t T,
                                    float *box_params, void *stream) {
    if (N == 0 || n_obj == 0) return NLR_OK;
    NLR_CHECK_ARG(tracks && timestamps && box_params, "track_box_params: NULL tensor");
    NLR_CHECK_ARG(T >= 2, "track_box_params: get_pose blends two recorded poses, T = %u", T);
    const size_t tot = (size_t)N * n_obj;
    hipLaunchKernelGGL(nlr_track_box_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tracks, timestamps, N,
                       n_obj, T, box_params);
    NLR_LAUNCH_CHECK("nlr_track_box_kernel");
    return NLR_OK;
}

// ---- adjoint of "tracks -> box-frame points and directions of the owned samples" (track refinement, train.py:244-268) ---------
// One lane per owned sample.  The lane repeats the forward of its (ray, track) pair - records and weight from nlr_track_records,
// blended pose, cos / sin, scale - and turns the cotangents of its point and direction into the 7 pose gradients.  Written on
// q = p_w - center: the reference's rotation, quirk included, is linear in the point, so rot(p_w) + rot(-center) = rot(q).
// The reduction never sends one value per sample to memory:
//   (1) the list is sorted by (ray, sample), so the samples of one (ray, track) pair lie in one or a few stretches of adjacent
//       lanes: a segmented shuffle reduction leaves each stretch's sum with its first lane inside the wave;
//   (2) that lane splits it by w1 / 1 - w1 onto the two records and adds the 14 values into the workgroup's LDS slot table
//       [n_obj][T][7] (ds_add_f32: almost all runs of a workgroup land on the same few slots);
//   (3) the workgroup writes its table as one slab of the workspace, and nlr_obj_frame_sum_kernel adds the slabs in a fixed order.
// A slot table beyond NLR_OBJB_SLOTS floats of LDS (large n_obj * T) skips (2) and (3): the run heads add into the zeroed g_tracks
// with global atomics, one per (run, record, column).
#define NLR_OBJB_SLOTS 39936      // floats of LDS for the largest slot table (156 KiB of the CU's 160 KiB) ...
#define NLR_OBJB_SLOTS_SMALL 4096 // ... and for the usual one (16 KiB: several workgroups share a CU)
#define NLR_OBJB_MAX_BLOCKS 256   // slabs (one per CU of an MI355X): contiguous shares of the list, so a workgroup meets few (ray, track) pairs more than once

struct ObjFrameBwd {
    const float *tracks, *ts, *origins, *dirs, *viewdirs, *tdist;
    uint32_t N, S, n_obj, T;
    const int32_t *ray_idx, *sample_idx, *track_idx;
    uint32_t K, per_block;  // samples per workgroup (multiple of 256)
    const float *g_pts, *g_dirs;
};

// SLOTS: capacity of the LDS slot table in floats, 0 = no table (run heads add into g_tracks)
template <int SLOTS>
__global__ void __launch_bounds__(256) nlr_obj_frame_bwd_kernel(ObjFrameBwd a, float *__restrict__ out) {
    constexpr bool LDS_SLOTS = SLOTS > 0;
    __shared__ float slots[LDS_SLOTS ? SLOTS : 1];
    const uint32_t n_slots = a.n_obj * a.T * 7;
    if (LDS_SLOTS) {
        for (uint32_t i = threadIdx.x; i < n_slots; i += 256) slots[i] = 0.0f;
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t lo = blockIdx.x * a.per_block, hi = lo + a.per_block < a.K ? lo + a.per_block : a.K;
    for (uint32_t base = lo; base < hi; base += 256) {  // (uniform trip count per workgroup: the shuffles below see whole waves)
        const uint32_t k = base + threadIdx.x;
        bool valid = k < hi;
        uint32_t ray = 0, smp = 0, o = 0;
        if (valid) {
            ray = (uint32_t)a.ray_idx[k];
            smp = (uint32_t)a.sample_idx[k];
            o = (uint32_t)a.track_idx[k];
            valid = ray < a.N && smp < a.S && o < a.n_obj;  // an index outside the batch contributes nothing
        }
        float g[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t i1 = 0, i2 = 0;
        float w1 = 0.0f;
        if (valid) {
            float pw[3], q[3], vd[3], gp[3], gd[3];
            const TrackBox t = nlr_track_box(a.tracks + (size_t)o * a.T * 9, a.T, a.ts[ray]);
            i1 = t.i1, i2 = t.i2, w1 = t.w1;
            const float cs = t.b0[0], sn = t.b0[1], sc[3] = {t.b1[1], t.b1[2], t.b1[3]};
            nlr_interval_midpoint(a.tdist, a.origins, a.dirs, a.S, ray, smp, pw);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                q[c] = pw[c] - t.pose[c];
                vd[c] = a.viewdirs[(size_t)ray * 3 + c];
                gp[c] = a.g_pts[(size_t)k * 3 + c];
                gd[c] = a.g_dirs[(size_t)k * 3 + c];
            }
            float g_cs = 0.0f, g_sn = 0.0f, g_sc[3];
            // p = scale * u, u = (cs q0 - sn q1, sn ux + cs q1, q2)
            float ux, uy;
            nlr_rotate_yaw(cs, sn, q[0], q[1], ux, uy);
            g_sc[0] = gp[0] * ux;
            g_sc[1] = gp[1] * uy;
            g_sc[2] = gp[2] * q[2];
            const float guy = gp[1] * sc[1], gux = gp[0] * sc[0] + sn * guy;
            g_sn += ux * guy - q[1] * gux;
            g_cs += q[1] * guy + q[0] * gux;
            g[0] = -(cs * gux);
            g[1] = -(cs * guy - sn * gux);
            g[2] = -(gp[2] * sc[2]);
            // dir = e / |e|, e = scale * v, v = (cs d0 - sn d1, sn vx + cs d1, d2)
            float vx, vy;
            nlr_rotate_yaw(cs, sn, vd[0], vd[1], vx, vy);
            const float e[3] = {sc[0] * vx, sc[1] * vy, sc[2] * vd[2]};
            const float inv = 1.0f / sqrtf((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
            const float n[3] = {e[0] * inv, e[1] * inv, e[2] * inv};
            const float dot = (n[0] * gd[0] + n[1] * gd[1]) + n[2] * gd[2];
            float ge[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) ge[c] = (gd[c] - n[c] * dot) * inv;
            g_sc[0] += ge[0] * vx;
            g_sc[1] += ge[1] * vy;
            g_sc[2] += ge[2] * vd[2];
            const float gvy = ge[1] * sc[1], gvx = ge[0] * sc[0] + sn * gvy;
            g_sn += vx * gvy - vd[1] * gvx;
            g_cs += vd[1] * gvy + vd[0] * gvx;
            g[3] = cs * g_sn - sn * g_cs;
#pragma unroll
            for (int c = 0; c < 3; ++c) g[4 + c] = g_sc[c] * (-0.5f * sc[c] * sc[c]);  // scale = 1 / (wlh / 2 + 1e-9)
        }
        // (1) segmented reduction over the runs of equal (ray, track) inside the wave.  A run is a stretch of ADJACENT lanes: along a
        // ray the owner can change and come back (a box inside another), so lanes are matched by run number, not by (ray, track).
        const uint32_t key_r = valid ? ray : 0xffffffffu, key_o = valid ? o : 0xffffffffu;
        const uint32_t prev_r = __shfl_up(key_r, 1, 64), prev_o = __shfl_up(key_o, 1, 64);
        const bool first = lane == 0 || prev_r != key_r || prev_o != key_o;
        const uint32_t run = (uint32_t)__popcll(__ballot(first) & ((2ull << lane) - 1ull));  // number of run starts up to this lane
        const bool head = valid && first;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const bool same = __shfl_down(run, d, 64) == run && lane + d < 64;
#pragma unroll
            for (int c = 0; c < 7; ++c) {
                const float v = __shfl_down(g[c], d, 64);
                g[c] += same ? v : 0.0f;
            }
        }
        // (2) the run's sum onto its two records
        if (head) {
            const size_t r1 = (size_t)o * a.T + i1, r2 = (size_t)o * a.T + i2;
#pragma unroll
            for (int c = 0; c < 7; ++c) {
                if (LDS_SLOTS) {
                    atomicAdd(&slots[r1 * 7 + c], w1 * g[c]);
                    atomicAdd(&slots[r2 * 7 + c], (1.0f - w1) * g[c]);
                } else {
                    atomicAdd(out + r1 * 9 + c, w1 * g[c]);
                    atomicAdd(out + r2 * 9 + c, (1.0f - w1) * g[c]);
                }
            }
        }
    }
    if (LDS_SLOTS) {  // (3) the workgroup's slab
        __syncthreads();
        float *slab = out + (size_t)blockIdx.x * n_slots;
        for (uint32_t i = threadIdx.x; i < n_slots; i += 256) slab[i] = slots[i];
    }
}

// g_tracks [n_obj * T, 9]: columns 0..6 = the sum of the slabs in slab order, columns 7 and 8 = 0
__global__ void __launch_bounds__(256) nlr_obj_frame_sum_kernel(const float *__restrict__ slabs, uint32_t n_slabs, uint32_t n_rec,
                                                               float *__restrict__ g_tracks) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec * 9) return;
    const uint32_t rec = i / 9, c = i - rec * 9;
    float s = 0.0f;
    if (c < 7)
        for (uint32_t b = 0; b < n_slabs; ++b) s += slabs[(size_t)b * n_rec * 7 + rec * 7 + c];
    g_tracks[i] = s;
}

static inline uint32_t obj_frame_blocks(uint32_t K) {
    const uint32_t nb = (K + 255) / 256;
    return nb < NLR_OBJB_MAX_BLOCKS ? nb : NLR_OBJB_MAX_BLOCKS;
}

extern "C" size_t nlr_obj_frame_backward_workspace_bytes(uint32_t K, uint32_t n_obj, uint32_t T) {
    const size_t n_slots = (size_t)n_obj * T * 7;
    if (K == 0 || n_slots == 0 || n_slots > NLR_OBJB_SLOTS) return 0;  // (the large-table path adds into g_tracks directly)
    return (size_t)obj_frame_blocks(K) * n_slots * sizeof(float);
}

extern "C" int nlr_obj_frame_backward(const float *tracks, const float *timestamps, const float *origins, const float *directions,
                                      const float *viewdirs, const float *tdist, uint32_t N, uint32_t S, uint32_t n_obj, uint32_t T,
                                      const int32_t *ray_idx, const int32_t *sample_idx, const int32_t *track_idx, uint32_t K,
                                      const float *g_pts, const float *g_dirs, float *g_tracks, void *workspace, size_t workspace_bytes,
                                      void *stream) {
    if (n_obj == 0 || T == 0) return NLR_OK;
    NLR_CHECK_ARG(g_tracks, "obj_frame_backward: g_tracks is NULL");
    hipStream_t st = (hipStream_t)stream;
    const size_t n_rec = (size_t)n_obj * T, n_slots = n_rec * 7;
    NLR_CHECK_ARG(n_rec * 9 < (1ull << 31), "obj_frame_backward: n_obj * T = %zu records do not fit the 32-bit slot index", n_rec);
    if (K == 0) {
        NLR_HIP(hipMemsetAsync(g_tracks, 0, n_rec * 9 * sizeof(float), st));
        return NLR_OK;
    }
    NLR_CHECK_ARG(tracks && timestamps && origins && directions && viewdirs && tdist && ray_idx && sample_idx && track_idx && g_pts && g_dirs,
                  "obj_frame_backward: NULL tensor");
    NLR_CHECK_ARG(T >= 2, "obj_frame_backward: get_pose blends two recorded poses, T = %u", T);
    NLR_CHECK_ARG(N >= 1 && S >= 1, "obj_frame_backward: %u owned samples of an empty batch (N = %u, S = %u)", K, N, S);
    NLR_CHECK_ARG(K < (1u << 31), "obj_frame_backward: K = %u owned samples do not fit the 32-bit list index", K);
    const uint32_t nb = obj_frame_blocks(K);
    ObjFrameBwd a;
    a.tracks = tracks;
    a.ts = timestamps;
    a.origins = origins;
    a.dirs = directions;
    a.viewdirs = viewdirs;
    a.tdist = tdist;
    a.N = N;
    a.S = S;
    a.n_obj = n_obj;
    a.T = T;
    a.ray_idx = ray_idx;
    a.sample_idx = sample_idx;
    a.track_idx = track_idx;
    a.K = K;
    a.per_block = (uint32_t)((((size_t)K + nb - 1) / nb + 255) / 256 * 256);
    a.g_pts = g_pts;
    a.g_dirs = g_dirs;
    if (n_slots <= NLR_OBJB_SLOTS) {
        const size_t need = nlr_obj_frame_backward_workspace_bytes(K, n_obj, T);
        if (!workspace || workspace_bytes < need)
            NLR_FAIL(NLR_ERR_WORKSPACE, "obj_frame_backward: workspace %zu B < nlr_obj_frame_backward_workspace_bytes() = %zu B", workspace_bytes,
                     need);
        if (n_slots <= NLR_OBJB_SLOTS_SMALL)
            hipLaunchKernelGGL(nlr_obj_frame_bwd_kernel<NLR_OBJB_SLOTS_SMALL>, dim3(nb), dim3(256), 0, st, a, (float *)workspace);
        else
            hipLaunchKernelGGL(nlr_obj_frame_bwd_kernel<NLR_OBJB_SLOTS>, dim3(nb), dim3(256), 0, st, a, (float *)workspace);
        NLR_LAUNCH_CHECK("nlr_obj_frame_bwd_kernel");
        hipLaunchKernelGGL(nlr_obj_frame_sum_kernel, dim3((unsigned)((n_rec * 9 + 255) / 256)), dim3(256), 0, st, (const float *)workspace, nb,
                           (uint32_t)n_rec, g_tracks);
        NLR_LAUNCH_CHECK("nlr_obj_frame_sum_kernel");
    } else {
        NLR_HIP(hipMemsetAsync(g_tracks, 0, n_rec * 9 * sizeof(float), st));
        hipLaunchKernelGGL(nlr_obj_frame_bwd_kernel<0>, dim3(nb), dim3(256), 0, st, a, g_tracks);
        NLR_LAUNCH_CHECK("nlr_obj_frame_bwd_kernel");
    }
    return NLR_OK;
}

// ---- adjoint of "rays -> box-frame points and directions of the owned samples" (pose refinement with objects) -----------------
// The sibling of nlr_obj_frame_bwd_kernel: the same map (nlr_box_coords / nlr_box_dir), differentiated by the ray instead of the
// track.  Here the box record of every (ray, track) is data (box_params), and the result is per RAY: a ray's owned samples are one
// contiguous stretch of the (ray, sample)-sorted list, so each output row is the sum of one stretch and nothing is shared between
// rays - no atomics, no workspace, and an order of additions that the list alone decides.
//   Lanes: one 16-lane DPP row per ray, 16 rays per workgroup.  A stretch is at most S <= 128 entries and most rays own none: a
//   whole wave per ray would idle 48 of its lanes on a typical stretch (and 64 on an empty one), a lane per ray would walk its
//   stretch alone with its neighbours reading far-apart parts of the list.  The row finds its stretch itself - two 17-ary searches
//   in ray_idx, the 16 lanes probing 16 split points per step (6 steps for 1.5 M entries, against 21 of a binary search) - walks it
//   16 entries per trip (lane r takes entries r, r + 16, ... of the stretch: adjacent lanes read adjacent entries) and adds the 16
//   partial sums with the DPP butterfly of the row.
template <int CTRL>
__device__ __forceinline__ float nlr_obj_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
// sum over the 16 lanes of a row, every lane gets the same bits (a + b == b + a at every step)
__device__ __forceinline__ float nlr_obj_row_sum(float v) {
    v += nlr_obj_dpp<0xB1>(v);   // quad_perm [1,0,3,2]
    v += nlr_obj_dpp<0x4E>(v);   // quad_perm [2,3,0,1]
    v += nlr_obj_dpp<0x141>(v);  // row_half_mirror
    v += nlr_obj_dpp<0x140>(v);  // row_mirror
    return v;
}
// First index in the sorted ray_idx[lo, hi) whose entry is not below `key`, found by the 16 lanes r of a row together (`shift` = the
// row's first lane in the wave).  Every probe lies inside [lo, hi); the range shrinks at every step whatever the list holds.
__device__ __forceinline__ uint32_t nlr_obj_row_lower_bound(const int32_t *__restrict__ ray_idx, uint32_t lo, uint32_t hi, int32_t key,
                                                            uint32_t r, uint32_t shift) {
    while (lo < hi) {
        const uint32_t len = hi - lo, step = len / 17 + 1;
        auto probe = [&](uint32_t j) {  // split point j = 0..15, non-decreasing in j
            const uint32_t d = step * (j + 1) - 1;
            return lo + (d < len - 1 ? d : len - 1);
        };
        const bool below = ray_idx[probe(r)] < key;
        const uint32_t c = (uint32_t)__popc((uint32_t)(__ballot(below) >> shift) & 0xffffu);  // probes below the key: the first c
        const uint32_t nlo = c ? probe(c - 1) + 1 : lo, nhi = c < 16 ? probe(c) : hi;
        lo = nlo;
        hi = nhi;
    }
    return lo;
}

struct ObjFrameBwdRays {
    const float *box, *viewdirs, *tdist;
    uint32_t N, S, n_obj;
    const int32_t *ray_idx, *sample_idx, *track_idx;
    uint32_t K;
    const float *g_pts, *g_dirs;
    float *d_origins, *d_dirs, *d_viewdirs;
};

__global__ void __launch_bounds__(256) nlr_obj_frame_bwd_rays_kernel(ObjFrameBwdRays a) {
    const uint32_t r = threadIdx.x & 15, shift = threadIdx.x & 48;
    const uint32_t ray = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (ray >= a.N) return;  // (whole rows)
    // the ray's stretch [lo, hi) of the list
    uint32_t lo = nlr_obj_row_lower_bound(a.ray_idx, 0, a.K, (int32_t)ray, r, shift), hi = lo;
    if (lo < a.K && a.ray_idx[lo] == (int32_t)ray) {
        uint32_t cap = lo + a.S < a.K ? lo + a.S : a.K;  // a ray owns at most S samples: the stretch ends inside [lo, lo + S] ...
        if (cap < a.K && a.ray_idx[cap] <= (int32_t)ray) cap = a.K;  // ... of a list made by nonzero(); any other list: search to its end
        hi = nlr_obj_row_lower_bound(a.ray_idx, lo + 1, cap, (int32_t)ray + 1, r, shift);
    }
    const bool want_p = a.d_origins || a.d_dirs, want_v = a.d_viewdirs != nullptr;
    float go[3] = {0.0f, 0.0f, 0.0f}, gd_[3] = {0.0f, 0.0f, 0.0f}, gv[3] = {0.0f, 0.0f, 0.0f};
    float vd[3] = {0.0f, 0.0f, 0.0f};
    if (want_v && lo < hi) {
#pragma unroll
        for (int c = 0; c < 3; ++c) vd[c] = a.viewdirs[(size_t)ray * 3 + c];
    }
    for (uint32_t k = lo + r; k < hi; k += 16) {
        const uint32_t smp = (uint32_t)a.sample_idx[k], o = (uint32_t)a.track_idx[k];
        if (smp >= a.S || o >= a.n_obj) continue;  // an index outside the batch contributes nothing
        const f32x4 *b = reinterpret_cast<const f32x4 *>(a.box + ((size_t)ray * a.n_obj + o) * 8);  // (32-byte records of a float array)
        const f32x4 b0 = b[0], b1 = b[1];
        const float cs = b0[0], sn = b0[1], sc[3] = {b1[1], b1[2], b1[3]};
        if (want_p) {  // p = scale * (rot(t_mid d + o) + t_w_o)
            const float t0 = a.tdist[(size_t)ray * (a.S + 1) + smp], t1 = a.tdist[(size_t)ray * (a.S + 1) + smp + 1];
            const float tm = 0.5f * (t0 + t1);
            float gp[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) gp[c] = a.g_pts[(size_t)k * 3 + c];
            const float gy = gp[1] * sc[1], gx = gp[0] * sc[0] + sn * gy;
            const float gq[3] = {cs * gx, cs * gy - sn * gx, gp[2] * sc[2]};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                go[c] += gq[c];
                gd_[c] += tm * gq[c];
            }
        }
        if (want_v) {  // dir = e / |e|, e = scale * rot(v)
            float g[3], vx, vy;
#pragma unroll
            for (int c = 0; c < 3; ++c) g[c] = a.g_dirs[(size_t)k * 3 + c];
            nlr_rotate_yaw(cs, sn, vd[0], vd[1], vx, vy);
            const float e[3] = {sc[0] * vx, sc[1] * vy, sc[2] * vd[2]};
            const float inv = 1.0f / sqrtf((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
            const float n[3] = {e[0] * inv, e[1] * inv, e[2] * inv};
            const float dot = (n[0] * g[0] + n[1] * g[1]) + n[2] * g[2];
            float ge[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) ge[c] = (g[c] - n[c] * dot) * inv;
            const float hy = ge[1] * sc[1], hx = ge[0] * sc[0] + sn * hy;
            gv[0] += cs * hx;
            gv[1] += cs * hy - sn * hx;
            gv[2] += ge[2] * sc[2];
        }
    }
    // the row's sums (whole rows arrive here together: ray, lo and hi are the same in the 16 lanes); lane c < 3 writes component c
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        go[c] = nlr_obj_row_sum(go[c]);
        gd_[c] = nlr_obj_row_sum(gd_[c]);
        gv[c] = nlr_obj_row_sum(gv[c]);
    }
    if (r < 3) {
        const size_t i = (size_t)ray * 3 + r;
        if (a.d_origins) a.d_origins[i] = r == 0 ? go[0] : r == 1 ? go[1] : go[2];
        if (a.d_dirs) a.d_dirs[i] = r == 0 ? gd_[0] : r == 1 ? gd_[1] : gd_[2];
        if (a.d_viewdirs) a.d_viewdirs[i] = r == 0 ? gv[0] : r == 1 ? gv[1] : gv[2];
    }
}

extern "C" int nlr_obj_frame_backward_rays(const float *box_params, const float *viewdirs, const float *tdist, uint32_t N, uint32_t S,
                                           uint32_t n_obj, const int32_t *ray_idx, const int32_t *sample_idx, const int32_t *track_idx,
                                           uint32_t K, const float *g_pts, const float *g_dirs, float *d_origins, float *d_directions,
                                           float *d_viewdirs, void *stream) {
    if (N == 0 || (!d_origins && !d_directions && !d_viewdirs)) return NLR_OK;
    hipStream_t st = (hipStream_t)stream;
    NLR_CHECK_ARG((size_t)N * 3 < (1ull << 32), "obj_frame_backward_rays: N = %u rays do not fit the 32-bit row index", N);
    if (K == 0) {
        for (float *d : {d_origins, d_directions, d_viewdirs})
            if (d) NLR_HIP(hipMemsetAsync(d, 0, (size_t)N * 3 * sizeof(float), st));
        return NLR_OK;
    }
    NLR_CHECK_ARG(box_params && tdist && ray_idx && sample_idx && track_idx, "obj_frame_backward_rays: NULL tensor");
    NLR_CHECK_ARG(((uintptr_t)box_params & 15) == 0, "obj_frame_backward_rays: box_params must be 16-byte aligned");
    NLR_CHECK_ARG(g_pts || (!d_origins && !d_directions), "obj_frame_backward_rays: g_pts is NULL");
    NLR_CHECK_ARG((g_dirs && viewdirs) || !d_viewdirs, "obj_frame_backward_rays: d_viewdirs needs g_dirs and viewdirs");
    NLR_CHECK_ARG(S >= 1 && n_obj >= 1, "obj_frame_backward_rays: %u owned samples of an empty batch (S = %u, n_obj = %u)", K, S, n_obj);
    NLR_CHECK_ARG(K < (1u << 31) - 2 * S, "obj_frame_backward_rays: K = %u owned samples do not fit the 32-bit list index", K);
    ObjFrameBwdRays a;
    a.box = box_params;
    a.viewdirs = viewdirs;
    a.tdist = tdist;
    a.N = N;
    a.S = S;
    a.n_obj = n_obj;
    a.ray_idx = ray_idx;
    a.sample_idx = sample_idx;
    a.track_idx = track_idx;
    a.K = K;
    a.g_pts = g_pts;
    a.g_dirs = g_dirs;
    a.d_origins = d_origins;
    a.d_dirs = d_directions;
    a.d_viewdirs = d_viewdirs;
    hipLaunchKernelGGL(nlr_obj_frame_bwd_rays_kernel, dim3((N + 15) / 16), dim3(256), 0, st, a);
    NLR_LAUNCH_CHECK("nlr_obj_frame_bwd_rays_kernel");
    return NLR_OK;
}

// ---- owner of every sample + per-class lists of the owned samples ---------------------------------------------------------
// nlr_box_owner_kernel is the one owner map of the library: nlr_box_winner launches it with n_classes = 0 for the map alone.
// Three small kernels and no atomics (device-scope atomics on one counter serialise at the memory side across the 8 XCDs:
// 10 k of them cost more than the rest of the branch): (1) owner map + the number of owned samples of every class in every
// wave, (2) exclusive scan of those counts per class, (3) scatter.  The lists come out in sample order.
//   lists[c * cap + i] = flat sample index (ray * S + k), counts[c] = length.
__global__ void __launch_bounds__(256) nlr_box_owner_kernel(const float *__restrict__ tdist, const float *__restrict__ origins,
                                                           const float *__restrict__ dirs, const float *__restrict__ box, uint32_t N,
                                                           uint32_t S, uint32_t n_obj, const int32_t *__restrict__ track_class,
                                                           uint32_t n_classes, int32_t *__restrict__ winner,
                                                           uint32_t *__restrict__ wave_counts) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;  // (N * S < 2^32, checked by the host: no 64-bit division here)
    const bool in = i < N * S;
    int32_t w = -1;
    if (in) {
        const uint32_t ray = i / S, k = i - ray * S;
        float p[3];
        nlr_interval_midpoint(tdist, origins, dirs, S, ray, k, p);
        const f32x4 *b = reinterpret_cast<const f32x4 *>(box + (size_t)ray * n_obj * 8);  // (32-byte records of a float array)
        // four boxes per trip: their eight 16-byte loads are issued together, and the inside test is branch-free
        for (uint32_t o0 = 0; o0 < n_obj; o0 += 4) {
            f32x4 b0[4], b1[4];
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) {
                const uint32_t o = o0 + u < n_obj ? o0 + u : n_obj - 1;
                b0[u] = b[2 * o];
                b1[u] = b[2 * o + 1];
            }
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) {
                float x[3];
                nlr_box_coords(b0[u], b1[u], p, x);
                const int inside = nlr_box_inside(x) & (int)(o0 + u < n_obj);
                w = inside ? (int32_t)(o0 + u) : w;
            }
        }
        winner[i] = w;
    }
    if (n_classes == 0) return;  // (nlr_box_winner: the owner map alone, no track_class and no count buffer)
    const int32_t cls = w >= 0 ? track_class[w] : -1;
    const uint32_t lane = threadIdx.x & 63, gw = i >> 6;
    for (uint32_t c = 0; c < n_classes; ++c) {
        const uint64_t mask = __ballot(cls == (int32_t)c);
        if (lane == 0) wave_counts[(size_t)c * gridDim.x * 4 + gw] = (uint32_t)__popcll(mask);
    }
}

extern "C" int nlr_box_winner(const float *tdist, const float *origins, const float *directions, const float *box_params, uint32_t N,
                              uint32_t S, uint32_t n_obj, int32_t *winner, void *stream) {
    if (N == 0 || S == 0) return NLR_OK;
    NLR_CHECK_ARG(tdist && origins && directions && winner && (box_params || n_obj == 0), "box_winner: NULL tensor");
    const size_t M = (size_t)N * S;
    NLR_CHECK_ARG(M < (1ull << 32), "box_winner: N * S = %zu does not fit the 32-bit sample index", M);
    hipLaunchKernelGGL(nlr_box_owner_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tdist, origins, directions,
                       box_params, N, S, n_obj, (const int32_t *)nullptr, 0u, winner, (uint32_t *)nullptr);
    NLR_LAUNCH_CHECK("nlr_box_owner_kernel");
    return NLR_OK;
}

// exclusive scan of one class's per-wave counts (blockIdx.x = class), in place; counts[c] = total
__global__ void __launch_bounds__(1024) nlr_obj_scan_kernel(uint32_t *__restrict__ wave_counts, uint32_t nw, uint32_t *__restrict__ counts) {
    __shared__ uint32_t part[1024];
    uint32_t *wc = wave_counts + (size_t)blockIdx.x * nw;  // nw is a multiple of 4 and the slab 16-byte aligned: 16-byte accesses
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const uint32_t per = (((nw + 1023) / 1024) + 3) & ~3u, lo = threadIdx.x * per, hi = lo + per < nw ? lo + per : nw;
    uint32_t sum = 0;
    for (uint32_t j = lo; j < hi; j += 4) {
        const u32x4 v = *reinterpret_cast<const u32x4 *>(wc + j);
        sum += (v[0] + v[1]) + (v[2] + v[3]);
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {  // Hillis-Steele inclusive scan of the 1024 partial sums
        const uint32_t v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;
    for (uint32_t j = lo; j < hi; j += 4) {
        const u32x4 v = *reinterpret_cast<const u32x4 *>(wc + j);
        u32x4 o;
        o[0] = run;
        o[1] = o[0] + v[0];
        o[2] = o[1] + v[1];
        o[3] = o[2] + v[2];
        run = o[3] + v[3];
        *reinterpret_cast<u32x4 *>(wc + j) = o;
    }
    if (threadIdx.x == 1023) counts[blockIdx.x] = part[1023];
}

__global__ void __launch_bounds__(256) nlr_obj_scatter_kernel(const int32_t *__restrict__ winner, const int32_t *__restrict__ track_class,
                                                             uint32_t M, uint32_t n_classes, const uint32_t *__restrict__ wave_offsets,
                                                             uint32_t *__restrict__ lists, uint32_t cap) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t w = i < M ? winner[i] : -1;
    const int32_t cls = w >= 0 ? track_class[w] : -1;
    const uint32_t lane = threadIdx.x & 63, gw = i >> 6;
    if (__ballot(cls >= 0) == 0) return;
    for (uint32_t c = 0; c < n_classes; ++c) {
        const uint64_t mask = __ballot(cls == (int32_t)c);
        if (cls == (int32_t)c)
            lists[(size_t)c * cap + wave_offsets[(size_t)c * gridDim.x * 4 + gw] + __popcll(mask & ((1ull << lane) - 1ull))] = i;
    }
}

// ---- one class's network on its list -------------------------------------------------------------------------------------
// One lane per owned sample, 64 samples per wave, 3 waves per workgroup, one workgroup per CU.  The class's weights (78 KB for
// the shipped ObjMLP) are copied into LDS once per workgroup, transposed ([input][output], outputs padded to 64 / 32 / 4): a
// weight row is read with wave-uniform ds_read_b128s (broadcast) and feeds packed-f32 FMAs whose 64 / 32 accumulators - the
// layer's outputs - stay in VGPRs.  A layer's inputs are walked by the running input index: grid features and direction
// encoding from registers (compile-time loops), the latent code from the track's row in memory, the previous layer's outputs
// from the wave's [feature][lane] slab in LDS (written only after the layer that reads the old contents has finished: the
// outputs wait in registers, so one 64-feature and one 32-feature slab per wave are enough).
struct ObjNet {
    GridParams gp;
    const float *wpack;       // dev: all weight matrices + biases as the kernel's LDS image
    uint32_t wfloats;         // its size (multiple of 4)
    uint32_t o_d0, o_d2, o_v[NLR_OBJ_MAX_DEPTH], o_rgb;        // weight offsets (floats) inside the image
    uint32_t o_bd0, o_bd2, o_bv[NLR_OBJ_MAX_DEPTH], o_brgb;    // bias offsets
    const float *latents;     // [n_tracks, latent_size]
    uint32_t n_grid, lat_size, lat_shape, lat_tex, lat_tex_off, BW, W, D, skip, deg, DE;
    float density_bias, premul, rgb_bias, rgb_pad;
    int32_t class_type;
    __host__ __device__ ObjCols cols() const { return nlr_obj_cols(n_grid, BW, DE, D, W); }  // columns of acts / gacts (training form)
};

struct ObjApply {
    const uint32_t *lists, *counts;  // [n_classes][cap], [n_classes]
    uint32_t cap;
    const int32_t *winner;
    const float *tdist, *origins, *dirs, *viewdirs, *box;
    uint32_t N, S, n_obj, K;
    float *density, *rgb, *sem;
};

#define NLR_OBJ_WAVES 3  // (NLR_OBJ_WMAX, the floats of LDS for the weight image: nlr_obj_layers.h)

template <int OUT>
__device__ __forceinline__ void obj_fma_row(float (&acc)[OUT], const float *wrow, float x) {
#pragma unroll
    for (int o = 0; o < OUT; o += 4) {
        const f32x4 w = *reinterpret_cast<const f32x4 *>(wrow + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[o + e] = fmaf(w[e], x, acc[o + e]);
    }
}
// inputs from the wave's LDS slab [k][lane]
template <int OUT>
__device__ __forceinline__ void obj_seg_lds(float (&acc)[OUT], const float *w, uint32_t row0, uint32_t n, const float *slab, uint32_t lane) {
    const float *wr = w + (size_t)row0 * OUT;
#pragma unroll 2
    for (uint32_t k = 0; k < n; ++k) obj_fma_row<OUT>(acc, wr + (size_t)k * OUT, slab[k * 64 + lane]);
}
// inputs from a per-lane row in memory (the track's latent code)
template <int OUT>
__device__ __forceinline__ void obj_seg_mem(float (&acc)[OUT], const float *w, uint32_t row0, uint32_t n, const float *x) {
    const float *wr = w + (size_t)row0 * OUT;
#pragma unroll 2
    for (uint32_t k = 0; k < n; ++k) obj_fma_row<OUT>(acc, wr + (size_t)k * OUT, x[k]);
}
// inputs from registers
template <int OUT, int NR>
__device__ __forceinline__ void obj_seg_reg(float (&acc)[OUT], const float *w, uint32_t row0, uint32_t n, const float (&x)[NR]) {
    const float *wr = w + (size_t)row0 * OUT;
#pragma unroll
    for (int k = 0; k < NR; ++k)
        if ((uint32_t)k < n) obj_fma_row<OUT>(acc, wr + (size_t)k * OUT, x[k]);
}

// The accumulator chain of a Linear - the ONE numerical difference between the two kernels.  Every output is one fused-multiply-add
// chain over the inputs in their order.  BIAS_LAST = false (rendering): the chain starts at the bias.  BIAS_LAST = true (training):
// it starts at zero and the bias is added after the last input - the reference's own order of operations.  At these widths
// (K = 64 .. 175) torch's Linear on the CPU (the f32 GEMM the reference runs) was observed to sum that way (DESIGN, round-4
// f-1 x f-3): restated so an output has the reference's bits, where the chain started at the bias is a few ulp of the hidden units
// away.  Under the x1500 density gain of a trained-like field those ulp are 2e-5 of a density, which the resampler of the next level
// turns into moved sample positions: training is held to the reference's step, so its forward sums as the reference does.
template <bool BIAS_LAST, int OUT>
__device__ __forceinline__ void obj_begin(float (&acc)[OUT], const float *b) {
#pragma unroll
    for (int o = 0; o < OUT; ++o) acc[o] = BIAS_LAST ? 0.0f : b[o];
}
template <bool BIAS_LAST, int OUT>
__device__ __forceinline__ void obj_end(float (&acc)[OUT], const float *b) {
    if (!BIAS_LAST) return;
#pragma unroll
    for (int o = 0; o < OUT; ++o) acc[o] = acc[o] + b[o];
}

template <typename T, int C, int LMAX>
__global__ void __launch_bounds__(64 * NLR_OBJ_WAVES) nlr_objmlp_kernel(const ObjNet *__restrict__ nets, ObjApply a) {
    // blockIdx.y = class: the workgroups of a class with few (or no) owned samples leave at once and their CUs go to the others
    const ObjNet &net = nets[blockIdx.y];
    const uint32_t *list = a.lists + (size_t)blockIdx.y * a.cap;
    __shared__ __attribute__((aligned(16))) float wl[NLR_OBJ_WMAX];
    __shared__ float slab_a[NLR_OBJ_WAVES][64 * 64];  // trunk hidden, then the bottleneck
    __shared__ float slab_v[NLR_OBJ_WAVES][32 * 64];  // view layers
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t count = a.counts[blockIdx.y];
    if (blockIdx.x * (64 * NLR_OBJ_WAVES) >= count) return;  // (the whole workgroup: nothing to do)
    for (uint32_t i = threadIdx.x * 4; i < net.wfloats; i += 64 * NLR_OBJ_WAVES * 4)
        *reinterpret_cast<f32x4 *>(wl + i) = *reinterpret_cast<const f32x4 *>(net.wpack + i);
    __syncthreads();
    float *sa = slab_a[wave], *sv = slab_v[wave];
    const bool want_rgb = a.rgb != nullptr;
    for (uint32_t base = (blockIdx.x * NLR_OBJ_WAVES + wave) * 64; base < count; base += gridDim.x * (64 * NLR_OBJ_WAVES)) {
        const bool valid = base + lane < count;
        const uint32_t m = list[valid ? base + lane : count - 1];
        const uint32_t ray = m / a.S, k = m - ray * a.S;
        // ---- box coordinates of the interval midpoint, obj_utils.py:158-176,203-216
        float pw[3], po[3];
        nlr_interval_midpoint(a.tdist, a.origins, a.dirs, a.S, ray, k, pw);
        const uint32_t tr = (uint32_t)a.winner[m];
        const f32x4 *b = reinterpret_cast<const f32x4 *>(a.box + ((size_t)ray * a.n_obj + tr) * 8);  // (32-byte records of a float array)
        const f32x4 b0 = b[0], b1 = b[1];
        nlr_box_coords(b0, b1, pw, po);
        Gauss g;  // GridEncoder(bound = 1): (x + 1) / 2 (grid.py:162)
        g.x0 = (po[0] + 1.0f) / 2.0f;
        g.x1 = (po[1] + 1.0f) / 2.0f;
        g.x2 = (po[2] + 1.0f) / 2.0f;
        g.zs = 0.0f;
        float de[3], ds0[3 * NLR_OBJ_MAX_DEG], ds1[3 * NLR_OBJ_MAX_DEG];  // [x | sin(2^j x) | sin(2^j x + pi/2)], j-major
        if (want_rgb) {  // view direction in the box frame, normalised (obj_utils.py:171-176), then pos_enc (coord.py:199-210)
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
        // ---- grid features (gridencoder.cu:87-199 on the box coordinates)
        float gf[LMAX * C];
#pragma unroll
        for (int l = 0; l < LMAX; ++l) {
            float acc[C];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = 0.0f;
            if ((uint32_t)l < net.gp.L) nlr_level_accum<T, C>(net.gp, l, g, 1.0f, acc);
#pragma unroll
            for (int c = 0; c < C; ++c) gf[l * C + c] = acc[c];
        }
        const float *lat = net.latents + (size_t)tr * net.lat_size;
        // ---- density_layer: [grid | shape latent] -> 64 -> ReLU -> bottleneck (models.py:887-889,996-1003)
        {
            float h[64];
            obj_begin<false, 64>(h, wl + net.o_bd0);
            obj_seg_reg<64, LMAX * C>(h, wl + net.o_d0, 0, net.n_grid, gf);
            obj_seg_mem<64>(h, wl + net.o_d0, net.n_grid, net.lat_shape, lat);
#pragma unroll
            for (int o = 0; o < 64; ++o) sa[o * 64 + lane] = fmaxf(h[o], 0.0f);
        }
        float x[64];
        if (want_rgb) {
            obj_begin<false, 64>(x, wl + net.o_bd2);
            obj_seg_lds<64>(x, wl + net.o_d2, 0, 64, sa, lane);
        } else {  // proposal levels replace the density only: output 0 of density_layer.2
            float r = wl[net.o_bd2];
            for (uint32_t kk = 0; kk < 64; ++kk) r = fmaf(wl[net.o_d2 + kk * 64], sa[kk * 64 + lane], r);
            x[0] = r;
        }
        {
            const float xd = x[0] + net.density_bias;
            if (valid) a.density[m] = xd > 20.0f ? xd : log1pf(expf(xd));  // F.softplus, models.py:1116
        }
        if (valid && a.sem) {  // fixed_semantic: one-hot of the class (models.py:1124-1130)
            for (uint32_t c = 0; c < a.K; ++c) a.sem[(size_t)c * a.N * a.S + m] = ((int32_t)c == net.class_type) ? 1.0f : 0.0f;
        }
        if (!want_rgb) continue;
#pragma unroll
        for (int o = 0; o < 64; ++o) sa[o * 64 + lane] = x[o];  // (every read of the hidden units above has completed: same wave)
        // ---- view MLP: inputs = [bottleneck | dir enc | texture latent] (models.py:1190-1234)
        const float *lat_tex = lat + net.lat_tex_off;
        for (uint32_t i = 0; i < net.D; ++i) {
            float h[32];
            const float *wv = wl + net.o_v[i];
            obj_begin<false, 32>(h, wl + net.o_bv[i]);
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
#pragma unroll
            for (int o = 0; o < 32; ++o) sv[o * 64 + lane] = fmaxf(h[o], 0.0f);
        }
        float c4[4];
        const float *wr = wl + net.o_rgb;
        obj_begin<false, 4>(c4, wl + net.o_brgb);
        obj_seg_lds<4>(c4, wr, 0, net.W, sv, lane);
        if (net.D - 1 == net.skip) {
            obj_seg_lds<4>(c4, wr, net.W, net.BW, sa, lane);
            obj_seg_reg<4, 3>(c4, wr, net.W + net.BW, 3, de);
            obj_seg_reg<4, 3 * NLR_OBJ_MAX_DEG>(c4, wr, net.W + net.BW + 3, 3 * net.deg, ds0);
            obj_seg_reg<4, 3 * NLR_OBJ_MAX_DEG>(c4, wr, net.W + net.BW + 3 + 3 * net.deg, 3 * net.deg, ds1);
            obj_seg_mem<4>(c4, wr, net.W + net.BW + net.DE, net.lat_tex, lat_tex);
        }
        if (valid) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {  // models.py:1251-1255
                const float sg = 1.0f / (1.0f + expf(-(net.premul * c4[c] + net.rgb_bias)));
                a.rgb[(size_t)c * a.N * a.S + m] = sg * (1.0f + 2.0f * net.rgb_pad) - net.rgb_pad;
            }
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
struct NlrObjects {
    std::vector<ObjLayers> layers;  // the layer table of every class: what cls' offsets are made of
    std::vector<ObjNet> cls;
    ObjNet *nets_dev = nullptr;  // the same, as the kernel reads them
    std::vector<void *> allocs;
    int32_t *track_class = nullptr;  // dev
    uint32_t n_tracks = 0;
    int device = 0;
    uint32_t cus = 0;
    ~NlrObjects() {
        for (void *p : allocs) (void)hipFree(p);
    }
};

// a device buffer of the object set: a copy of `host`, or zeros where host is NULL
static int obj_upload(NlrObjects *o, const void *host, size_t bytes, void **out, hipStream_t st) {
    void *p = nullptr;
    NLR_HIP(hipMalloc(&p, bytes ? bytes : 16));
    o->allocs.push_back(p);
    if (!host) NLR_HIP(hipMemsetAsync(p, 0, bytes ? bytes : 16, st));
    else if (bytes) NLR_HIP(hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, st));
    NLR_HIP(hipStreamSynchronize(st));  // the sources are temporaries
    *out = p;
    return NLR_OK;
}

// Step 1 of making an object set, "lay out and allocate": the layer table of every class (nlr_obj_layers: envelope and offsets),
// its grid parameters and ObjNet, the track classes, a zeroed latent table and zeroed weight images on the device.  The training plan
// stops here (its images are filled from the flat buffers by nlr_obj_train_pack, its latent table from the caller's tensor).
static int obj_layout(const NlrObjectsDesc *d, const char *who, std::unique_ptr<NlrObjects> &own, hipStream_t st) {
    NLR_CHECK_ARG(d->n_classes >= 1 && d->n_classes <= NLR_OBJ_MAX_CLASSES && d->classes, "%s: n_classes = %u outside [1,%d]", who, d->n_classes,
                  NLR_OBJ_MAX_CLASSES);
    NLR_CHECK_ARG(d->n_tracks >= 1 && d->track_class, "%s: no tracks", who);
    own.reset(new NlrObjects());
    NlrObjects *o = own.get();
    int rc = NLR_OK;
    NLR_HIP(hipGetDevice(&o->device));
    int cus = 0;
    NLR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, o->device));
    o->cus = (uint32_t)cus;
    o->n_tracks = d->n_tracks;
    const uint32_t lat_size = d->classes[0].latent_size;
    for (uint32_t t = 0; t < d->n_tracks; ++t)
        NLR_CHECK_ARG(d->track_class[t] >= 0 && (uint32_t)d->track_class[t] < d->n_classes, "objects_create: track_class[%u] = %d outside [0,%u)", t,
                      d->track_class[t], d->n_classes);
    if ((rc = obj_upload(o, d->track_class, (size_t)d->n_tracks * 4, (void **)&o->track_class, st))) return rc;
    float *lat_dev = nullptr;
    if (lat_size && (rc = obj_upload(o, nullptr, (size_t)d->n_tracks * lat_size * 4, (void **)&lat_dev, st))) return rc;
    o->cls.resize(d->n_classes);
    o->layers.resize(d->n_classes);
    for (uint32_t c = 0; c < d->n_classes; ++c) {
        const NlrObjClassDesc &cd = d->classes[c];
        const NlrMlpDesc &md = cd.mlp;
        ObjNet &n = o->cls[c];
        ObjLayers &t = o->layers[c];
        memset(&n, 0, sizeof(n));
        char msg[256];
        if (cd.latent_size != lat_size)
            NLR_FAIL(NLR_ERR_UNSUPPORTED, "objects_create: classes disagree on latent_size (%u vs %u)", cd.latent_size, lat_size);
        if (!nlr_obj_layers(cd, who, c, t, msg, sizeof(msg))) NLR_FAIL(NLR_ERR_UNSUPPORTED, "%s", msg);
        if (!(md.grid.table_dtype == 0 || md.grid.table_dtype == 1)) NLR_FAIL(NLR_ERR_UNSUPPORTED, "objects_create: table dtype");
        if (!((md.grid.level_dim == 2 && md.grid.num_levels <= 8) || (md.grid.level_dim == 4 && md.grid.num_levels <= 4) ||
              (md.grid.level_dim == 1 && md.grid.num_levels <= 16)))
            NLR_FAIL(NLR_ERR_UNSUPPORTED, "objects_create: grid L=%u C=%u not supported by the object kernel", md.grid.num_levels, md.grid.level_dim);
        if (md.grid.level_dim != d->classes[0].mlp.grid.level_dim || md.grid.table_dtype != d->classes[0].mlp.grid.table_dtype)
            NLR_FAIL(NLR_ERR_UNSUPPORTED,
                     "objects_create: the classes' grids must share level_dim and table dtype (one kernel instance serves them all)");
        if ((rc = nlr_fill_grid_params(&n.gp, md.grid.table, md.grid.table_dtype, md.grid.offsets, md.grid.num_levels, md.grid.level_dim,
                                       md.grid.log2_per_level_scale, md.grid.base_resolution, md.grid.gridtype, (int)md.grid.align_corners,
                                       md.grid.interp)))
            return rc;
        n.n_grid = t.n_grid, n.lat_size = lat_size, n.lat_shape = t.lat_shape, n.lat_tex = t.lat_tex, n.lat_tex_off = t.lat_tex_off;
        n.BW = t.BW, n.W = t.W, n.D = t.D, n.skip = t.skip, n.deg = t.deg, n.DE = t.DE;
        n.density_bias = md.density_bias, n.premul = md.rgb_premultiplier, n.rgb_bias = md.rgb_bias, n.rgb_pad = md.rgb_padding;
        n.class_type = cd.class_type;
        n.latents = lat_dev;
        // the image's offsets: Linear i of the table is density_layer.0, density_layer.2, lin_second_stage_0 .. D-1, rgb_layer
        const ObjLinear *L = t.lin;
        n.o_d0 = L[0].img_w, n.o_bd0 = L[0].img_b, n.o_d2 = L[1].img_w, n.o_bd2 = L[1].img_b;
        for (uint32_t i = 0; i < t.D; ++i) n.o_v[i] = L[2 + i].img_w, n.o_bv[i] = L[2 + i].img_b;
        n.o_rgb = L[2 + t.D].img_w, n.o_brgb = L[2 + t.D].img_b;
        n.wfloats = t.img_floats;
        if ((rc = obj_upload(o, nullptr, (size_t)t.img_floats * 4, (void **)&n.wpack, st))) return rc;
    }
    return obj_upload(o, o->cls.data(), o->cls.size() * sizeof(ObjNet), (void **)&o->nets_dev, st);
}

// Step 2, "fill the images from NlrLinears": nn.Linear weight [out, in] -> [in][outp] at the table's place (the padding stays zero)
static int obj_fill_images(NlrObjects *o, const NlrObjectsDesc *d, hipStream_t st) {
    for (uint32_t c = 0; c < d->n_classes; ++c) {
        const NlrMlpDesc &md = d->classes[c].mlp;
        const ObjLayers &t = o->layers[c];
        std::vector<float> img(t.img_floats, 0.0f);
        for (uint32_t i = 0; i < t.n_lin; ++i) {
            const ObjLinear &L = t.lin[i];
            const NlrLinear &l = i == 0 ? md.density0 : i == 1 ? md.density2 : i == t.n_lin - 1 ? md.rgb_layer : md.view[i - 2];
            NLR_CHECK_ARG(l.weight && l.bias, "objects: %s weight/bias is NULL", L.name);
            NLR_CHECK_ARG(l.out_features == L.n_out && l.in_features == L.n_in, "objects: %s expected [%u,%u], got [%u,%u]", L.name, L.n_out,
                          L.n_in, l.out_features, l.in_features);
            for (uint32_t r = 0; r < L.n_out; ++r) {
                for (uint32_t k = 0; k < L.n_in; ++k) img[L.img_w + (size_t)k * L.outp + r] = l.weight[(size_t)r * L.n_in + k];
                img[L.img_b + r] = l.bias[r];
            }
        }
        NLR_HIP(hipMemcpyAsync(const_cast<float *>(o->cls[c].wpack), img.data(), img.size() * 4, hipMemcpyHostToDevice, st));
        NLR_HIP(hipStreamSynchronize(st));  // the source is a temporary
    }
    return NLR_OK;
}

extern "C" int nlr_objects_create(const NlrObjectsDesc *d, NlrObjects **out, void *stream) {
    NLR_CHECK_ARG(d && out, "objects_create: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    std::unique_ptr<NlrObjects> own;
    int rc = obj_layout(d, "objects_create", own, st);
    if (rc) return rc;
    const uint32_t lat_size = d->classes[0].latent_size;
    if (lat_size) {
        NLR_CHECK_ARG(d->latents, "objects_create: latent_size = %u but latents is NULL", lat_size);
        NLR_HIP(hipMemcpyAsync(const_cast<float *>(own->cls[0].latents), d->latents, (size_t)d->n_tracks * lat_size * 4, hipMemcpyHostToDevice, st));
        NLR_HIP(hipStreamSynchronize(st));
    }
    if ((rc = obj_fill_images(own.get(), d, st))) return rc;
    *out = own.release();
    return NLR_OK;
}

extern "C" void nlr_objects_destroy(NlrObjects *o) { delete o; }

// ---- launch preparation, shared by nlr_objects_apply and the training form ------------------------------------------------------
// The workspace: [counts | owner map | per-class lists | per-wave counts / offsets] and, for the training backward,
// [acts aw x M | gacts gw x M | slabs slices x classes x stride | totals classes x stride] f32.  Every piece starts on a 256-byte
// boundary; `bytes` is what the pieces take with the slack for aligning the caller's pointer (workspace NULL: the size alone).
struct ObjWorkspace {
    uint32_t *counts, *lists, *wave_counts;
    int32_t *winner;
    float *acts, *gacts, *slabs, *totals;
    size_t bytes;
};
static ObjWorkspace obj_carve(void *workspace, size_t nc, uint32_t N, uint32_t S, uint32_t aw, uint32_t gw, size_t slab_floats, size_t total_floats) {
    const size_t M = (size_t)N * S, nw = ((M + 255) / 256) * 4;
    const uintptr_t p0 = ((uintptr_t)workspace + 255) & ~(uintptr_t)255;
    uintptr_t p = p0;
    auto take = [&p](size_t b) {
        const uintptr_t at = p;
        p += al(b);
        return at;
    };
    ObjWorkspace w;
    w.counts = (uint32_t *)take(256);
    w.winner = (int32_t *)take(M * 4);
    w.lists = (uint32_t *)take(nc * M * 4);
    w.wave_counts = (uint32_t *)take(nc * nw * 4);
    w.acts = (float *)take(M * aw * 4);  // (the four pieces of the backward are empty for a forward: all sizes 0)
    w.gacts = (float *)take(M * gw * 4);
    w.slabs = (float *)take(slab_floats * 4);
    w.totals = (float *)take(total_floats * 4);
    w.bytes = 256 + (size_t)(p - p0);
    return w;
}

extern "C" size_t nlr_objects_workspace_bytes(const NlrObjects *o, uint32_t N, uint32_t S) {
    return o ? obj_carve(nullptr, o->cls.size(), N, S, 0, 0, 0, 0).bytes : 0;
}

// owner map + per-class lists of the owned samples: owner -> scan -> scatter; the map is copied to winner_out when given
static int obj_make_lists(const NlrObjects *o, const ObjWorkspace &w, const NlrRays *rays, const float *tdist, const float *box_params, uint32_t N,
                          uint32_t S, uint32_t n_obj, int32_t *winner_out, hipStream_t st) {
    const size_t M = (size_t)N * S;
    const uint32_t nc = (uint32_t)o->cls.size(), nblk = (uint32_t)((M + 255) / 256), nw = nblk * 4;
    hipLaunchKernelGGL(nlr_box_owner_kernel, dim3(nblk), dim3(256), 0, st, tdist, rays->origins, rays->directions, box_params, N, S, n_obj,
                       o->track_class, nc, w.winner, w.wave_counts);
    NLR_LAUNCH_CHECK("nlr_box_owner_kernel");
    hipLaunchKernelGGL(nlr_obj_scan_kernel, dim3(nc), dim3(1024), 0, st, w.wave_counts, nw, w.counts);
    NLR_LAUNCH_CHECK("nlr_obj_scan_kernel");
    hipLaunchKernelGGL(nlr_obj_scatter_kernel, dim3(nblk), dim3(256), 0, st, w.winner, o->track_class, (uint32_t)M, nc, w.wave_counts, w.lists,
                       (uint32_t)M);
    NLR_LAUNCH_CHECK("nlr_obj_scatter_kernel");
    if (winner_out) NLR_HIP(hipMemcpyAsync(winner_out, w.winner, M * 4, hipMemcpyDeviceToDevice, st));
    return NLR_OK;
}

static ObjApply obj_apply_args(const ObjWorkspace &w, const NlrRays *rays, const float *tdist, const float *box_params, uint32_t N, uint32_t S,
                               uint32_t n_obj, float *density, float *rgb, float *semantic, uint32_t K) {
    return ObjApply{w.lists, w.counts, /*cap*/ N * S, w.winner, tdist, rays->origins, rays->directions, rays->viewdirs, box_params, N, S, n_obj,
                    /*K*/ semantic ? K : 0, density, rgb, semantic};
}

// the networks' grid: one launch, grid.y = class; persistent workgroups (at most one per CU) that read their class's count on the device
static dim3 obj_net_grid(const NlrObjects *o, uint32_t N, uint32_t S) {
    const size_t M = (size_t)N * S;
    const uint32_t per = 64 * NLR_OBJ_WAVES, nb = (uint32_t)((M + per - 1) / per);
    return dim3(o->cus < nb ? o->cus : nb, (uint32_t)o->cls.size());
}

int nlr_objects_apply_impl(const NlrObjects *o, const NlrRays *rays, const float *tdist, const float *box_params, uint32_t N, uint32_t S,
                           uint32_t n_obj, float *density, float *rgb, float *semantic, uint32_t K, int32_t *winner_out, void *workspace,
                           size_t workspace_bytes, hipStream_t st) {
    NLR_CHECK_ARG(o && rays && tdist && density, "objects_apply: NULL argument");
    if (N == 0 || S == 0 || n_obj == 0) return NLR_OK;
    NLR_CHECK_ARG(box_params, "objects_apply: box_params is NULL");
    NLR_CHECK_ARG(n_obj == o->n_tracks, "objects_apply: %u boxes per ray, the object set has %u tracks", n_obj, o->n_tracks);
    NLR_CHECK_ARG(rays->origins && rays->directions && (rays->viewdirs || !rgb), "objects_apply: ray batch has NULL origins/directions/viewdirs");
    const size_t need = nlr_objects_workspace_bytes(o, N, S);
    if (!workspace || workspace_bytes < need)
        NLR_FAIL(NLR_ERR_WORKSPACE, "objects_apply: workspace %zu B < nlr_objects_workspace_bytes() = %zu B", workspace_bytes, need);
    NLR_CHECK_ARG((size_t)N * S < (1ull << 32), "objects_apply: N * S = %zu does not fit the 32-bit sample index", (size_t)N * S);
    const ObjWorkspace w = obj_carve(workspace, o->cls.size(), N, S, 0, 0, 0, 0);
    int rc = obj_make_lists(o, w, rays, tdist, box_params, N, S, n_obj, winner_out, st);
    if (rc) return rc;
    const ObjApply a = obj_apply_args(w, rays, tdist, box_params, N, S, n_obj, density, rgb, semantic, K);
    const GridParams &gp0 = o->cls[0].gp;
#define OBJ_LAUNCH(C, LM)                                                                                                                 \
    if (gp0.table_dtype == 0) hipLaunchKernelGGL((nlr_objmlp_kernel<float, C, LM>), obj_net_grid(o, N, S), dim3(64 * NLR_OBJ_WAVES), 0, st, \
                                                 o->nets_dev, a);                                                                         \
    else hipLaunchKernelGGL((nlr_objmlp_kernel<__half, C, LM>), obj_net_grid(o, N, S), dim3(64 * NLR_OBJ_WAVES), 0, st, o->nets_dev, a)
    if (gp0.C == 2) { OBJ_LAUNCH(2, 8); }
    else if (gp0.C == 4) { OBJ_LAUNCH(4, 4); }
    else { OBJ_LAUNCH(1, 16); }
#undef OBJ_LAUNCH
    NLR_LAUNCH_CHECK("nlr_objmlp_kernel");
    return NLR_OK;
}

extern "C" int nlr_objects_apply(const NlrObjects *o, const NlrRays *rays, const float *tdist, const float *box_params, uint32_t N, uint32_t S,
                                 uint32_t n_obj, float *density, float *rgb, float *semantic, uint32_t K, int32_t *winner_out, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    return nlr_objects_apply_impl(o, rays, tdist, box_params, N, S, n_obj, density, rgb, semantic, K, winner_out, workspace, workspace_bytes,
                                  (hipStream_t)stream);
}

// ---- the training form of the branch: plan, forward, backward (header section 7e) ---------------------------------------------
#include "nlr_objects_train.h"
