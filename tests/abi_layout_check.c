/* Prints the layout the C compiler gives every struct of include/nerflidar_hip.h: one "Struct sizeof N" line and one
 * "Struct.field offset size" line per field.  tests/test_abi.py compares the lines with the ctypes classes of nerflidar_hip/_lib.py and
 * the field names with the header's text, so a field missing here, there or in the header fails the test. */
#include <stddef.h>
#include <stdio.h>

#include "nerflidar_hip.h"

#define S(T) printf(#T " sizeof %zu\n", sizeof(T))
#define F(T, f) printf(#T "." #f " %zu %zu\n", offsetof(T, f), sizeof(((T *)0)->f))

int main(void) {
    S(NlrLinear); F(NlrLinear, weight); F(NlrLinear, bias); F(NlrLinear, out_features); F(NlrLinear, in_features);

    S(NlrGridDesc); F(NlrGridDesc, table); F(NlrGridDesc, table_dtype); F(NlrGridDesc, num_levels); F(NlrGridDesc, level_dim);
    F(NlrGridDesc, base_resolution); F(NlrGridDesc, log2_per_level_scale); F(NlrGridDesc, offsets); F(NlrGridDesc, gridtype);
    F(NlrGridDesc, align_corners); F(NlrGridDesc, interp);

    S(NlrMlpDesc); F(NlrMlpDesc, grid); F(NlrMlpDesc, density0); F(NlrMlpDesc, density2); F(NlrMlpDesc, disable_rgb);
    F(NlrMlpDesc, bottleneck_width); F(NlrMlpDesc, net_depth_viewdirs); F(NlrMlpDesc, net_width_viewdirs); F(NlrMlpDesc, skip_layer_dir);
    F(NlrMlpDesc, deg_view); F(NlrMlpDesc, view); F(NlrMlpDesc, rgb_layer); F(NlrMlpDesc, use_semantic); F(NlrMlpDesc, no_sem_layer);
    F(NlrMlpDesc, class_num); F(NlrMlpDesc, sem0); F(NlrMlpDesc, sem2); F(NlrMlpDesc, use_intensity); F(NlrMlpDesc, int0);
    F(NlrMlpDesc, int2); F(NlrMlpDesc, density_bias); F(NlrMlpDesc, rgb_premultiplier); F(NlrMlpDesc, rgb_bias); F(NlrMlpDesc, rgb_padding);
    F(NlrMlpDesc, re_weights);

    S(NlrModelDesc); F(NlrModelDesc, num_levels); F(NlrModelDesc, num_samples); F(NlrModelDesc, mlps); F(NlrModelDesc, dilation_multiplier);
    F(NlrModelDesc, dilation_bias); F(NlrModelDesc, anneal_slope); F(NlrModelDesc, resample_padding); F(NlrModelDesc, power_lambda);
    F(NlrModelDesc, std_scale); F(NlrModelDesc, bg_intensity); F(NlrModelDesc, opaque_background); F(NlrModelDesc, mlp_precision);

    S(NlrRays); F(NlrRays, origins); F(NlrRays, directions); F(NlrRays, viewdirs); F(NlrRays, radii); F(NlrRays, near); F(NlrRays, far);
    F(NlrRays, base_x); F(NlrRays, base_y);

    S(NlrRenderCfg); F(NlrRenderCfg, train_frac); F(NlrRenderCfg, compute_extras); F(NlrRenderCfg, sample_n); F(NlrRenderCfg, sample_m);
    F(NlrRenderCfg, rand_jitter); F(NlrRenderCfg, rand_deg); F(NlrRenderCfg, scale_factor); F(NlrRenderCfg, shuffled_rays);

    S(NlrLevelOut); F(NlrLevelOut, sdist); F(NlrLevelOut, tdist); F(NlrLevelOut, weights); F(NlrLevelOut, density); F(NlrLevelOut, rgb);
    F(NlrLevelOut, semantic); F(NlrLevelOut, intensity); F(NlrLevelOut, depth); F(NlrLevelOut, r_rgb); F(NlrLevelOut, r_acc);
    F(NlrLevelOut, r_distance_mean); F(NlrLevelOut, r_distance_median); F(NlrLevelOut, r_distance_percentile_5);
    F(NlrLevelOut, r_distance_percentile_95);

    S(NlrOut); F(NlrOut, rgb); F(NlrOut, depth); F(NlrOut, semantic); F(NlrOut, intensity); F(NlrOut, acc); F(NlrOut, distance_mean);
    F(NlrOut, distance_median); F(NlrOut, distance_percentile_5); F(NlrOut, distance_percentile_95); F(NlrOut, labels); F(NlrOut, points);
    F(NlrOut, packed); F(NlrOut, packed_h); F(NlrOut, packed_w); F(NlrOut, history);

    S(NlrObjClassDesc); F(NlrObjClassDesc, mlp); F(NlrObjClassDesc, latent_size); F(NlrObjClassDesc, split_latent);
    F(NlrObjClassDesc, class_type);

    S(NlrObjectsDesc); F(NlrObjectsDesc, n_classes); F(NlrObjectsDesc, classes); F(NlrObjectsDesc, n_tracks); F(NlrObjectsDesc, track_class);
    F(NlrObjectsDesc, latents);
    return 0;
}
