/*
 * ppf_hip.hip — MI355X (gfx950) implementation of the C-ABI in include/ppf_hip.h.
 *
 * Path: A2 cloud sampling -> A3 pair feature + key hash -> A5-train model table ->
 * A5-match per-reference-point Hough vote over the discretised alpha -> argmax -> A8 pose assembly ->
 * A7 pose clustering.  Reference call sites: /root/reference/include/CloudProcessing.h:236
 * (trainModel), :442 (match), :495 (match_S2B).
 *
 * Data layout in HBM:
 *   clouds        SoA  x[] y[] z[] nx[] ny[] nz[]  (f32, coalesced 256 B per wave-instruction)
 *   slot map      slots/64 x {u64 occupancy bits, u32 rank, u32 pad}: hash slot -> dense bucket id
 *                 in one 16-byte load (the reference indexes 2^k slots by hash % slots and never
 *                 compares keys, so only "which slots are non-empty" has to be kept)
 *   bucket_off    n_tiles x (n_buckets+1) u32 CSR offsets, one CSR per accumulator tile
 *   records       pair records {row_a, row_b, alpha_a, alpha_b}: row = u32 code of the model ref's accumulator row (LDS byte
 *                 offset (guard + word_row*numAngles)*4, the half of the word its 16-bit cells use in bit 0, the entry's
 *                 count-table X and cell above bit 17: vote_row_code, agg_cell_bits), alpha = f32 alpha_m; 8 B per model
 *                 pair; per (tile, bucket) low-half rows first, bank- and phase-interleaved inside each half (see
 *                 place_entry); bucket_off counts records
 *   accumulator   LDS, ceil(tile_refs/2) x numAngles words of two 16-bit cells per workgroup (one workgroup = one scene
 *                 reference point x one tile of model reference points; 32-bit cells: one half of the tile's rows)
 *
 * This file is the one translation unit of libppf_hip.so; the code lives in the headers included at the bottom:
 *   kernels   ppf_train_kernels.h (table build)  ppf_sample_kernels.h (A2)  ppf_match_kernels.h (k_frames / k_pairs /
 *             k_group / k_vote)  ppf_pose_kernels.h (k_finalize, k_rank, clustering)  ppf_icp_kernels.h  ppf_prep_kernels.h
 *             ppf_depth_kernels.h  ppf_depth_normals_kernels.h  ppf_verify_kernels.h  ppf_render_kernels.h  ppf_select_kernels.h  ppf_refine_kernels.h
 *             ppf_register_kernels.h  ppf_plane_kernels.h  ppf_label_kernels.h  ppf_cluster_kernels.h  ppf_region_kernels.h  ppf_filter_kernels.h
 *             ppf_segment_kernels.h  ppf_edge_kernels.h  ppf_recognize_kernels.h  ppf_history_kernels.h  ppf_motion_kernels.h
 *             ppf_volume_kernels.h  ppf_volume_mesh_kernels.h  ppf_mesh_kernels.h  ppf_mesh_components_kernels.h
 *   host      ppf_device_mem.h (errors, block cache)  ppf_host_common.h (scans, sorts, model / workspace structs)
 *             ppf_model_host.h  ppf_match_host.h  ppf_batch_host.h  ppf_icp_host.h  ppf_stage_host.h (what every stage call
 *             shares: FrameRun, stage_finish, stage_entry)  ppf_prep_host.h (the segmented preparation stages; ppf_prep_* = one
 *             segment)  ppf_frame_host.h (ppf_prep_frame = their chain)
 *             ppf_match_frame_host.h  ppf_depthimage_host.h  ppf_depth_host.h  ppf_posetable_host.h  ppf_verify_host.h  ppf_render_host.h
 *             ppf_select_host.h  ppf_refine_host.h  ppf_register_host.h  ppf_plane_host.h  ppf_cluster_host.h  ppf_region_host.h
 *             ppf_filter_host.h  ppf_segment_host.h  ppf_edge_host.h  ppf_recognize_host.h  ppf_history_host.h  ppf_motion_host.h
 *             ppf_volume_host.h  ppf_mesh_components_host.h  ppf_mesh_host.h  (the C-ABI)
 *   model host (ppf_model_host.h): model_plan (parameters -> steps, slots, tiles; pure), build_table (training's device
 *             passes in named steps), ModelImage (what a model file holds: read + validate, write, download, upload),
 *             row_groups (the group records; pure), model_finish (what training and loading derive once the table stands)
 *
 * Compile: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared (see __graft_entry__.build()).
 * No CPU fallback exists: without a HIP device the compute entry points return PPF_ERR_HIP.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ppf_hip.h"
#include "ppf_core.h"

#include "ppf_device_mem.h"    /* fail(), HIPCHK, DevPool, DevBuf */
#include "ppf_train_kernels.h" /* accumulator geometry, CloudSoA, table-build kernels, scan */
#include "ppf_sample_kernels.h"
#include "ppf_match_kernels.h"
#include "ppf_icp_kernels.h"
#include "ppf_prep_kernels.h"
#include "ppf_depth_kernels.h" /* k_depth_count, k_depth_scatter */
#include "ppf_depth_normals_kernels.h" /* k_depth_normals, k_depthn_count, k_depthn_scatter */
#include "ppf_filter_kernels.h" /* k_depth_filter */
#include "ppf_edge_kernels.h" /* k_depth_edges, k_edge_select, k_edge_write */
#include "ppf_history_kernels.h" /* k_history_push */
#include "ppf_verify_kernels.h" /* k_vfy_grid_count / _grid_scatter, k_vfy_score, k_vfy_finish */
#include "ppf_render_kernels.h" /* k_rnd_window, k_rnd_splat, k_rnd_vfy_score, k_rnd_splat_frame, k_rnd_resolve */
#include "ppf_select_kernels.h" /* k_sel_mask, k_sel_key, k_sel_overlap, k_sel_greedy, k_sel_report, k_sel_paint */
#include "ppf_refine_kernels.h" /* k_rfn_refine */
#include "ppf_motion_kernels.h" /* k_motion_level0, k_motion_down, k_motion_maps, k_motion_eval, k_motion_group, k_motion_tail */
#include "ppf_volume_kernels.h" /* k_volume_fill, k_volume_integrate, k_volume_raycast, k_volume_cross */
#include "ppf_volume_mesh_kernels.h" /* k_vmesh_cells, k_vmesh_edges, k_vmesh_vertices, k_vmesh_triangles */
#include "ppf_mesh_kernels.h" /* k_mesh_tri, k_mesh_area, k_mesh_sample, k_mesh_draw_small / _large, k_mesh_visible, k_mesh_scatter */
#include "ppf_register_kernels.h" /* k_reg_rays, k_reg_clear, k_reg_draw, k_reg_resolve */
#include "ppf_plane_kernels.h" /* k_pln_hyp, k_pln_count, k_pln_best, k_pln_sum / _finish, k_pln_flags, k_pln_compact, k_pln_gather */
#include "ppf_label_kernels.h" /* uf_find, uf_unite, uf_root, cells_lower_bound, wave_max_by_key: no kernel */
#include "ppf_mesh_components_kernels.h" /* k_mc_init, k_mc_unite, k_mc_flatten, k_mc_tris, k_mc_edges, k_mc_comps, k_mc_rank, k_mc_flags, k_mc_write_* */
#include "ppf_cluster_kernels.h" /* k_clu_bounds, k_clu_grid, k_clu_keys, k_clu_runs, k_clu_cells, k_clu_link, k_clu_flatten ... k_clu_reduce */
#include "ppf_segment_kernels.h" /* k_seg_classify, k_seg_tile, k_seg_merge, k_seg_flatten, k_seg_valid, k_seg_rank, k_seg_labels */
#include "ppf_recognize_kernels.h" /* k_rec_dmax, k_rec_build, k_rec_popcount, k_rec_score, k_rec_finish */
#include "ppf_region_kernels.h" /* k_reg_runs, k_reg_link, k_reg_flatten, k_reg_attach */
#include "ppf_pose_kernels.h"  /* k_finalize, k_rank, clustering, result blocks */
#include "ppf_host_common.h"   /* scans, sorts, sampling, ppf_model / ppf_workspace, enqueue_cluster */
#include "ppf_model_host.h"    /* C-ABI: defaults, training, handles, model file */
#include "ppf_match_host.h"    /* C-ABI: workspaces, ppf_match_device, ppf_match, ppf_raw_votes, clustering */
#include "ppf_batch_host.h"    /* C-ABI: crops x models */
#include "ppf_icp_host.h"      /* row N2: ICP refinement, host side */
#include "ppf_stage_host.h"    /* what every stage call shares: FrameRun, frame_scan, frame_sort, stage_finish, stage_entry */
#include "ppf_prep_host.h"     /* row N4: the segmented cloud stages, ppf_prep_* (one segment each) */
#include "ppf_frame_host.h"    /* row N4 for all boxes of a frame: ppf_prep_frame, the chain of those stages */
#include "ppf_match_frame_host.h" /* match + ICP for all detections of a frame: ppf_match_frame */
#include "ppf_depthimage_host.h"  /* what the stages on a depth image share: checks, bindings, the outputs check */
#include "ppf_depth_host.h"       /* the scene cloud from a depth image: ppf_cloud_from_depth */
#include "ppf_posetable_host.h"   /* what the stages on a frame's pose table share: checks, render jobs, clears */
#include "ppf_verify_host.h"      /* pose verification of every detection of a frame: ppf_verify_frame */
#include "ppf_render_host.h"      /* surfel z-buffers: ppf_verify_frame_rendered, ppf_render_frame */
#include "ppf_select_host.h"      /* one consistent set of poses per frame: ppf_select_frame */
#include "ppf_refine_host.h"      /* refinement on the depth image itself: ppf_refine_frame */
#include "ppf_register_host.h"    /* a sensor depth image aligned to the colour camera: ppf_camera_*, ppf_depth_map, ppf_depth_register */
#include "ppf_plane_host.h"       /* a frame's support planes found and removed: ppf_prep_planes, ppf_prep_planes_apply */
#include "ppf_cluster_host.h"     /* a plane-free cloud split into object clusters: ppf_prep_clusters */
#include "ppf_region_host.h"      /* a cloud split into smooth surface regions: ppf_prep_regions */
#include "ppf_filter_host.h"      /* a depth image without flying pixels, smoothed inside each surface: ppf_depth_filter */
#include "ppf_history_host.h"     /* a camera's last frames fused into one depth image: ppf_depth_history_* */
#include "ppf_motion_host.h"      /* the camera's motion between two depth images: ppf_depth_motion */
#include "ppf_volume_host.h"      /* posed depth images fused into a TSDF volume: ppf_depth_volume_*, ppf_volume_mesh_* */
#include "ppf_mesh_components_host.h" /* a mesh's connected components, scraps removed: ppf_volume_mesh_upload, ppf_volume_mesh_components */
#include "ppf_mesh_host.h"        /* a model cloud sampled from a triangle mesh: ppf_cloud_from_mesh */
#include "ppf_segment_host.h"     /* a depth image's surfaces labelled in image space: ppf_depth_segments */
#include "ppf_edge_host.h"        /* a depth image's occluding and boundary edges, mask and edge cloud: ppf_depth_edges */
#include "ppf_recognize_host.h"   /* which trained models a proposal can be a view of: ppf_recognizer_*, ppf_recognize_frame */
