// Internal interface of the dynamic-object branch (nlr_objects.hip) used by the render loop (nlr_api.hip).
#pragma once
#include "nlr_common.h"
#include "nlr_obj_layers.h"

// workspace carving of both files: every slab starts on a 256-byte boundary
static inline size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

struct NlrObjects;
int nlr_objects_apply_impl(const NlrObjects *o, const NlrRays *rays, const float *tdist, const float *box_params, uint32_t N, uint32_t S,
                           uint32_t n_obj, float *density, float *rgb, float *semantic, uint32_t K, int32_t *winner_out, void *workspace,
                           size_t workspace_bytes, hipStream_t st);
