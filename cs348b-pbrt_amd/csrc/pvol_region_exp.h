// pvol_region_exp.h -- the second compilation of the kernels that march a medium (pvol_march_exp.hip, pvol_shoot_exp.hip): the same
// sources with ExponentialDensity::Density (volumes/exponential.h:58-62) as the density region instead of VolumeGridDensity::Density.
// The choice is made per translation unit, not per kernel or per call, so the kernels of the first compilation are what they were
// before the exponential medium existed (several sit at their VGPR limit) and the new ones carry no trilinear fetch.
// Everything the two units define with external linkage gets the suffix _exp here; the host picks a set by the scene's kind
// (pvol_launchers, pvol_host.h).  Kernels and launchers that never look at the medium (the merges, spec_compose, ...) are renamed as
// well, only to keep the two units apart at link time: the host keeps calling the first compilation's.
#ifndef PVOL_REGION_EXP_H
#define PVOL_REGION_EXP_H
#define PVOL_REGION_EXP 1
// kernels
#define li_seq_kernel li_seq_kernel_exp
#define li_par_kernel li_par_kernel_exp
#define li_resolve_kernel li_resolve_kernel_exp
#define li_replay_kernel li_replay_kernel_exp
#define li_geo_kernel li_geo_kernel_exp
#define li_resolve_lite_kernel li_resolve_lite_kernel_exp
#define li_group_kernel li_group_kernel_exp
#define li_fixup_kernel li_fixup_kernel_exp
#define li_fixup_group_kernel li_fixup_group_kernel_exp
#define lphoton_points_kernel lphoton_points_kernel_exp
#define stream_begin_kernel stream_begin_kernel_exp
#define surface_kernel surface_kernel_exp
#define spec_compose_kernel spec_compose_kernel_exp
#define spec_fill_kernel spec_fill_kernel_exp
#define tile_kernel tile_kernel_exp
#define tile_mw_kernel tile_mw_kernel_exp
#define shoot_kernel shoot_kernel_exp
#define merge_kernel merge_kernel_exp
#define merge_surface_kernel merge_surface_kernel_exp
#define place_rows_kernel place_rows_kernel_exp
#define single_seq_kernel single_seq_kernel_exp
#define single_par_kernel single_par_kernel_exp
#define single_stream_begin_kernel single_stream_begin_kernel_exp
// launchers and size helpers
#define pvol_launch_li_seq pvol_launch_li_seq_exp
#define pvol_launch_li_par pvol_launch_li_par_exp
#define pvol_launch_li_slice pvol_launch_li_slice_exp
#define pvol_launch_li_replay pvol_launch_li_replay_exp
#define pvol_launch_li_group pvol_launch_li_group_exp
#define pvol_launch_lphoton_points pvol_launch_lphoton_points_exp
#define pvol_launch_surface pvol_launch_surface_exp
#define pvol_launch_spec_compose pvol_launch_spec_compose_exp
#define pvol_launch_spec_fill pvol_launch_spec_fill_exp
#define pvol_launch_tile pvol_launch_tile_exp
#define pvol_group_lds_bytes pvol_group_lds_bytes_exp
#define pvol_fixgrp_lds_bytes pvol_fixgrp_lds_bytes_exp
#define pvol_tile_lds_bytes pvol_tile_lds_bytes_exp
#define pvol_launch_shoot pvol_launch_shoot_exp
#define pvol_launch_merge pvol_launch_merge_exp
#define pvol_launch_merge_surface pvol_launch_merge_surface_exp
#define pvol_launch_place_rows pvol_launch_place_rows_exp
#define pvol_shoot_state_words pvol_shoot_state_words_exp
#define pvol_launch_single_seq pvol_launch_single_seq_exp
#define pvol_launch_single_par pvol_launch_single_par_exp
// pvol_rays_dev.h (pvol_radiance_batch*) reads no density and is left out of the second compilation altogether (pvol_march.hip); its names
// stand here so that nothing of the sources compiled twice is off the list
#define rays_count_kernel rays_count_kernel_exp
#define rays_emit_kernel rays_emit_kernel_exp
#define rays_streams_kernel rays_streams_kernel_exp
#define rays_end_kernel rays_end_kernel_exp
#define rays_patch_kernel rays_patch_kernel_exp
#define rays_compose_kernel rays_compose_kernel_exp
#define pvol_launch_rays_count pvol_launch_rays_count_exp
#define pvol_launch_rays_emit pvol_launch_rays_emit_exp
#define pvol_launch_rays_patch pvol_launch_rays_patch_exp
#define pvol_launch_rays_compose pvol_launch_rays_compose_exp
#endif
