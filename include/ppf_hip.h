/*
 * ppf_hip.h — C-ABI of the MI355X-native PPF matching / voting engine (libppf_hip.so).
 *
 * This is the drop-in boundary for the one path the reference accelerates badly: everything
 * /root/reference/include/CloudProcessing.h does through cv::ppf_match_3d::PPF3DDetector.
 * Plain pointers and sizes only; no C++/torch/OpenCV/PCL types.  The header-only C++ facades
 * (include/ppf_match_3d.hpp — OpenCV-shaped, what the reference calls; include/ppf_pcl.hpp —
 * PCL-shaped, what BASELINE.json's north_star names) sit on top of exactly these entry points.
 *
 *   entry point                     replaces (reference call site)
 *   ------------------------------  ---------------------------------------------------------------
 *   ppf_model_train                 PPF3DDetector(relSampling, relDistance) + trainModel(Mat)
 *                                   CloudProcessing.h:205,217,234 (ctor), :236 (trainModel)
 *   ppf_model_retain/_release       by-value detector copies and explicit dtor calls
 *                                   CloudProcessing.h:81,206,218,240,432,485
 *   ppf_model_save / ppf_model_load detector.write(FileStorage) :250 / detector.read(FileNode) :112
 *   ppf_match                       detector.match(scene, results, step, dist) :442  (edge == NULL)
 *                                   detector.match_S2B(scene, edge, results, step, dist) :495
 *   ppf_raw_votes                   the per-reference-point argmax inside match() — the bit-exact
 *                                   parity surface {refIndMax, alphaIndMax, maxVotes}
 *   ppf_match_device (+workspace)   same as ppf_match with clouds already resident in HBM and an
 *                                   explicit HIP stream: the entry bench.py times
 *   ppf_match_batch                 the per-object loop around Matching (CloudProcessing.h:41-45 holds one cloud
 *                                   per detected object, :58 one detector per model): crops x models
 *   ppf_pair_features               pcl::PPFEstimation::compute (north_star's PCL names; the reference never calls it)
 *   ppf_sample_cloud                samplePCByQuantization inside trainModel/match (A2)
 *   ppf_transform_pc_pose           transformPCPose, src/YOLO_cropping_ppf_test.cpp:125
 *   ppf_icp_refine (+_device)       ICP icp(100, 0.005f, 2.5f, 8); icp.registerModelToScene(model, scene, poses)
 *                                   CloudProcessing.h:465-470 (Matching), :518-523 (Matching_S2B)
 *   ppf_icp_register                ICP::registerModelToScene(src, dst, residual, pose), the single-pose overload
 *   ppf_prep_crop / _voxel_grid /   CloudProcessor::SceneCropping :263, Subsampling :361, OutlierProcessing :341,
 *   _outlier_removal / _normals /   NormalEstimation :381, EdgeExtraction :406, PointCloudXYZNormalToMat :163
 *   _edges / _to_mat (+ppf_cloud_*) (the PCL stages that produce the matcher's input)
 *   ppf_match_frame                 match / match_S2B + ICP of every detection of a frame, ICP in one launch sequence
 *                                   (YOLO_cropping_ppf_test.cpp:88-127, CloudProcessing.h:495-523)
 *   ppf_prep_frame                  the same six stages for all of a frame's boxes at once (CloudProcessing.h:263-427
 *                                   return one cloud per detection)
 *   ppf_prep_planes (+_apply)       pcl::SACSegmentation + ExtractIndices, the step PPF pipelines take before cropping (the
 *                                   reference has none): the support planes of a frame found and removed
 *   ppf_cloud_from_depth (+_device) CloudProcessor::Deprojection(CameraIntr), an empty stub in the reference
 *                                   (CloudProcessing.h:262): the scene cloud from the depth image, Camera::back_projection
 *                                   (Camera.h:44-46) per valid pixel
 *   ppf_verify_frame                the `// TODO: Pose Validation` after `return *resultsSub[0];` of Matching and
 *                                   Matching_S2B (CloudProcessing.h:477-479, :530-532): scores every refined pose of
 *                                   every detection against its object cloud (and the depth image) and picks the best
 *   ppf_verify_frame_rendered       the same with self-occlusion: a model row counts only where it is visible in a surfel
 *                                   z-buffer of its own pose (the reference has no pose validation at all)
 *   ppf_render_frame                depth and instance-label images of the chosen poses, in place of the reference's
 *                                   transformPCPose -> writePLY dump of the result (YOLO_cropping_ppf_test.cpp:125-127)
 *   ppf_select_frame                one consistent set of poses per frame: duplicates and overlapping boxes suppressed,
 *                                   several instances per box kept (the reference returns `*resultsSub[0]` per box)
 *   ppf_refine_frame                poses fitted to the depth image itself (the reference stops at the ICP pose)
 *   ppf_depth_map_create +          k4a::transformation + depth_image_to_color_camera, the vendor SDK call the reference's
 *   ppf_depth_register (+_device)   grabber makes per capture (k4a_grabber.h:339-340, :391-392): a raw sensor depth image
 *                                   drawn into the colour camera's pixel grid, lens distortion of both cameras included
 *   ppf_camera_map_boxes            a detector's boxes on the raw colour image carried into that pixel grid
 *   ppf_depth_filter (+_device)     the depth clean-up a sensor pipeline runs before anything else (the reference has none):
 *                                   unsupported "flying" pixels removed, the others smoothed without crossing a depth step
 *   ppf_depth_motion (+_device)     the camera's rigid motion between two depth images (the reference's camera stands still):
 *                                   last frame's poses times it are this frame's start poses for ppf_refine_frame
 *   ppf_depth_segments (+_device)   detections without a detector, straight from the organised depth image (the reference takes
 *                                   its boxes from YOLO): the image's connected smooth surfaces as a label image and boxes
 *   ppf_recognize_frame             labels without a detector (the reference takes each crop's class from YOLO,
 *   (+ppf_recognizer_*)             YOLO_cropping_ppf_test.cpp:88-127): per proposal cloud a shortlist of the trained models
 *                                   it can be a view of, from the quantised pair features the models were trained on
 *
 * Conventions
 *   - A cloud argument is (pointer, rows, stride, normal_offset): float32 rows whose first three floats
 *     are x y z and whose normal sits `normal_offset` floats into the row; `stride` is the row pitch in
 *     floats.  The N x 6 CV_32FC1 Mat that CloudProcessing.h:163-190 builds is (6, PPF_NOFF_MAT = 3);
 *     a pcl::PointCloud<pcl::PointNormal> -- x y z 1 | nx ny nz 0 | curvature pad pad pad, the input of
 *     that function -- is (12, PPF_NOFF_PCL = 4).  Both host layouts pass without a repack.
 *   - Every function returns a ppf_status; no exception crosses this boundary.
 *     ppf_last_error() returns the calling thread's last message.
 *   - "No pose found" is not an error: *n_out = 0 (the wrapper handles it, :450-454).
 *   - Matching with an untrained/NULL model fails with PPF_ERR_NOT_TRAINED before any work
 *     (the wrapper's pre-check, :435-439).
 *   - Handles are immutable after training and reference counted: concurrent ppf_match calls
 *     on one model from several host threads / streams are safe; each call (or workspace)
 *     owns its scratch memory.
 *   - There is NO CPU fallback: without a usable HIP device every compute entry point
 *     returns PPF_ERR_HIP.
 */
#ifndef PPF_HIP_H
#define PPF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPF_ABI_VERSION 4 /* 4: every cloud argument carries its normal offset (pcl::PointNormal without a repack) */

#define PPF_NOFF_MAT 3 /* x y z nx ny nz */
#define PPF_NOFF_PCL 4 /* pcl::PointNormal: x y z pad nx ny nz pad curvature pad pad pad (stride 12) */

typedef enum ppf_status {
  PPF_OK = 0,
  PPF_ERR_INVALID = 1,     /* bad argument (CV_Assert in the reference's library) */
  PPF_ERR_NOT_TRAINED = 2, /* match on an untrained model */
  PPF_ERR_HIP = 3,         /* HIP runtime failure / no device */
  PPF_ERR_NOMEM = 4,
  PPF_ERR_IO = 5,
  PPF_ERR_CAPACITY = 6     /* caller's output buffer too small; *n_out holds the needed count */
} ppf_status;

typedef struct ppf_model ppf_model;         /* opaque, ref-counted, device-resident model table */
typedef struct ppf_workspace ppf_workspace; /* opaque per-caller scratch + result buffers */
typedef struct ppf_batch ppf_batch;         /* opaque: streams + workspaces of a batched call (crops x models) */
typedef struct ppf_cloud ppf_cloud;         /* opaque device-resident cloud: rows x y z nx ny nz + curvature */

typedef struct ppf_train_params {
  double relative_sampling_step;  /* PPF3DDetector ctor arg 1 (reference: 0.025, CloudProcessing.h:64) */
  double relative_distance_step;  /* ctor arg 2 (reference: 0.05, :65; TrainDetector default 0.5, :223) */
  double num_angles;              /* ctor arg 3, default 30 */
  int32_t presampled;             /* 1: rows are already the sampled model, skip samplePCByQuantization */
  int32_t distance_from_distance_step; /* 0 (default): distance step = diameter*relative_sampling_step,
                                          as the reference's library computes it; 1: use relative_distance_step */
  int32_t max_tile_refs;          /* 0 = auto: model reference points per LDS accumulator tile */
  int32_t key_equality;           /* PPF_KEY_BUCKET (0, the reference's library): a scene pair votes for every model pair
                                     in its hash bucket, colliding keys included; PPF_KEY_EXACT (1, PCL PPFHashMapSearch):
                                     only for model pairs with the same quantised key */
  int32_t feature;                /* PPF_FEATURE_PPF (0, the reference's library): three acos angles + distance, truncated;
                                     PPF_FEATURE_DARBOUX (1, PCL PPFEstimation / pcl::computePairFeatures): atan2 angle and
                                     two cosines of the Darboux frame + distance, keys floor(f / step).  A property of the
                                     trained table; matching follows the model. */
  int32_t reserved;               /* 0 */
} ppf_train_params;
#define PPF_KEY_BUCKET 0
#define PPF_KEY_EXACT 1
#define PPF_FEATURE_PPF 0
#define PPF_FEATURE_DARBOUX 1

typedef struct ppf_match_params {
  double relative_scene_sample_step; /* match() arg 3: every (int)(1/x)-th sampled scene point is a reference */
  double relative_scene_distance;    /* match() arg 4: scene sampling step, relative to the scene bbox */
  double position_threshold;         /* setSearchParams; < 0 = default (relative_sampling_step) */
  double rotation_threshold;         /* setSearchParams; < 0 = default ((360/angle_step)/180*pi) */
  int32_t use_weighted_avg;          /* setSearchParams */
  int32_t presampled;                /* 1: scene (and edge) rows are already sampled: every row votes */
  int32_t ref_offset;                /* sharding over ranks: vote reference points ref_offset, */
  int32_t ref_stride;                /*   ref_offset+ref_stride, ... of the reference list (1 = all) */
  int32_t skip_clustering;           /* 1: stop after per-reference poses */
  int32_t vote_mode;                 /* PPF_VOTE_AUTO (0): runs of many hits vote through per-run count tables;
                                        PPF_VOTE_DIRECT (1): every (entry, hit) pair casts its own atomic.  Same results. */
  /* PCL-semantics policy switches (pcl::PPFRegistration; zero = what the reference's library does) */
  double pair_radius;                /* > 0: a reference point is only paired with points at most this far away (PCL searches
                                        model_diameter / 2 around it); <= 0: with every point */
  int32_t rot_metric_relative;       /* 1: poses cluster when the angle of their RELATIVE rotation is below
                                        rotation_threshold (PCL); 0: when their rotation angles differ by less (OpenCV) */
  int32_t alpha_range_2pi;           /* 1: alpha_m - alpha_s is wrapped into [-pi, pi] and binned over 2 pi, numAngles bins of
                                        2 pi / numAngles (PCL); 0: the unwrapped difference over 4 pi (OpenCV) */
} ppf_match_params;
#define PPF_VOTE_AUTO 0
#define PPF_VOTE_DIRECT 1

/* cv::ppf_match_3d::Pose3D fields the reference reads (src/YOLO_cropping_ppf_test.cpp:124-125). */
typedef struct ppf_pose {
  double pose[16]; /* 4x4 row-major, model -> scene */
  double q[4];     /* quaternion [w x y z] */
  double t[3];
  double angle;
  double alpha;
  double residual;
  uint32_t model_index;
  uint32_t num_votes;
} ppf_pose;

/* argmax of one scene reference point's accumulator */
typedef struct ppf_vote {
  uint32_t ref_ind_max;
  uint32_t alpha_ind_max;
  uint32_t max_votes;
} ppf_vote;

typedef struct ppf_model_info {
  int32_t n_ref;         /* sampled model points N_m */
  int32_t num_angles;    /* floor(2*pi/angle_step) */
  uint32_t slots;        /* next_pow2(N_m^2) hash slots of the reference's table */
  uint32_t n_buckets;    /* non-empty slots */
  uint64_t n_entries;    /* N_m*(N_m-1) (+ spill duplicates) */
  int32_t n_tiles;       /* accumulator tiles */
  int32_t tile_refs;     /* model reference points per tile */
  double angle_step;     /* radians */
  double distance_step;  /* metres (float-rounded like the reference) */
  double diameter;       /* model bbox diagonal */
  double position_threshold_default;
  double rotation_threshold_default;
  uint64_t device_bytes; /* HBM held by the model */
} ppf_model_info;

/* counters of the last match executed in a workspace */
typedef struct ppf_match_stats {
  int32_t n_scene_sampled; /* rows after scene sampling */
  int32_t n_paired;        /* rows of the paired cloud (== n_scene_sampled unless S2B) */
  int32_t n_ref;           /* reference points voted by this call */
  int32_t n_poses;         /* clustered poses */
  uint64_t n_pairs;        /* scene pairs hashed and looked up */
  uint64_t n_votes;        /* accumulator increments == pair-matches */
  float ms_vote_kernel;    /* device time of the voting kernel, summed over the batches of the call (timing enabled) */
  float ms_pair_kernel;    /* pair kernel, likewise */
  float ms_total_device;   /* first kernel start -> last kernel end */
  float ms_group_kernel;   /* hit grouping (k_group, the two rankings, the count tables), likewise */
  uint64_t n_hits;         /* scene pairs that found a non-empty bucket */
  uint64_t n_lds_atomics;  /* LDS atomic lane-operations the voting kernel issued (<= n_votes when runs vote by counts) */
  uint64_t scratch_bytes;  /* device scratch of the call: hit pools, run table, frames */
  int32_t n_batches;       /* batches of reference points the call was cut into */
  int32_t n_retries;       /* repeats because the hit pools (sized from earlier calls) were too small */
  uint64_t n_acc32_items;  /* (reference point, accumulator tile)s voted with 32-bit cells: those whose 16-bit cells overflowed, or all
                              of them once a workspace has seen a twentieth of a call's votes cast twice (or with PPF_OPT_ACC32 = 1) */
  uint64_t n_tables;       /* count tables built for the runs of many hits (one per 191 hits of such a run) */
  uint64_t phase_clocks[8]; /* zero, except in a diagnostic build of the library (-DPPF_PHASE_CLOCKS): shader clocks the voting kernel's waves spent per phase */
} ppf_match_stats;

/* totals of one ppf_batch_run */
typedef struct ppf_batch_stats {
  uint64_t n_pairs, n_votes, n_hits, n_lds_atomics;
  int32_t n_matches; /* crops x models */
  int32_t n_retries;
  int32_t lanes;
  float ms_wall;     /* host wall clock of the call */
  /* with ppf_batch_enable_timing: device time of the kernels summed over all matches of the run (HIP events on each lane's
   * stream; lanes overlap, so the sums exceed the wall clock) */
  float ms_vote_kernel, ms_pair_kernel, ms_group_kernel;
  int32_t reserved;
} ppf_batch_stats;

/* cv::ppf_match_3d::ICP constructor arguments (uniform sampling, one correspondence per point) */
typedef struct ppf_icp_params {
  int32_t iterations;    /* ICP ctor arg 1 (reference: 100, CloudProcessing.h:465) */
  float tolerance;       /* arg 2 (0.005f) */
  float rejection_scale; /* arg 3 (2.5f); <= 0 disables the median+MAD rejection */
  int32_t num_levels;    /* arg 4 (8) */
  int32_t flags;         /* all poses of a call advance through the same launches, two per iteration, neighbours from a
                            grid search.  PPF_ICP_NO_SMALL_LEVELS, PPF_ICP_ONE_STREAM and PPF_ICP_LEGACY are accepted and
                            ignored: they selected an earlier schedule, since removed, that gave the same results. */
  int32_t reserved[3];
} ppf_icp_params;
#define PPF_ICP_NO_SMALL_LEVELS 1 /* accepted and ignored */
#define PPF_ICP_ONE_STREAM 2      /* accepted and ignored */
#define PPF_ICP_LEGACY 4          /* accepted and ignored */
#define PPF_ICP_GRID_ALWAYS 8 /* test knob: the grid neighbour search on every level (by default levels of at most 1,024 scene rows scan them all) */

void ppf_default_train_params(ppf_train_params* p);
void ppf_default_match_params(ppf_match_params* p);
void ppf_default_icp_params(ppf_icp_params* p); /* 100, 0.005f, 2.5f, 8: the reference's ICP object */
int ppf_abi_version(void);
/* copies the calling thread's last error text; returns its length */
int ppf_last_error(char* buf, int cap);
/* number of visible HIP devices (0 when there is none); never fails */
int ppf_device_count(void);

/* ---- model ------------------------------------------------------------------------------ */
ppf_status ppf_model_train(const float* xyzn, int n, int stride, int normal_offset, const ppf_train_params* params, ppf_model** out);
ppf_status ppf_model_retain(ppf_model* m);
ppf_status ppf_model_release(ppf_model* m);
ppf_status ppf_model_get_info(const ppf_model* m, ppf_model_info* info);
/* HIP device the model's table lives on (the current device of the thread that trained or loaded it) */
ppf_status ppf_model_get_device(const ppf_model* m, int* device);
/* pcl::PPFHashMapSearch::nearestNeighborSearch(f1, f2, f3, f4, indices) (north_star's PCL names; the reference never calls it):
 * the pairs (i, j) of the trained model's sampled points whose quantised feature equals the quantised f4[0..3] -- what a hash
 * map keyed on the quantised feature holds under that key -- ascending by (i, j), as pairs_ij[2q], pairs_ij[2q + 1].  The
 * feature kind and the steps are the model's (ppf_train_params.feature, ppf_model_info.angle_step / distance_step).
 * cap_pairs = 0 only counts (*n_out). */
ppf_status ppf_model_nearest_pairs(const ppf_model* m, const float* f4, uint32_t* pairs_ij, int cap_pairs, int* n_out);
/* The host-buffer entries (ppf_match, ppf_raw_votes, ppf_match_clouds) keep warm contexts with the model -- one per call that
 * has been in flight at once (at least 2, at most 16), each holding a stream, pinned staging and the scratch of its last call
 * (0.45 GB for a 50,000-point crop).  This releases the idle ones beyond `keep` (0: all) and returns how many went; calls in
 * flight are not touched, the next call on a model without an idle context simply starts cold.  The reference has no
 * counterpart: its detector frees nothing until it is destroyed (/root/reference/include/CloudProcessing.h:79-83). */
ppf_status ppf_model_trim_contexts(const ppf_model* m, int keep, int* released);
/* sampled model cloud (n_ref x 6 floats) */
ppf_status ppf_model_get_sampled(const ppf_model* m, float* out, int cap_rows);
/* CSR dump for inspection/tests: any pointer may be NULL. bucket_off has n_tiles*(n_buckets+1) u32,
 * entries n_entries x {int32 cell_base, float alpha_m}. */
ppf_status ppf_model_get_table(const ppf_model* m, uint32_t* bucket_slot, uint32_t* bucket_off, int32_t* entry_cell,
                               float* entry_alpha);
ppf_status ppf_model_save(const ppf_model* m, const char* path);
/* every field and table of the file is validated before use: a truncated or corrupt file is PPF_ERR_IO */
ppf_status ppf_model_load(const char* path, ppf_model** out);
/* The same byte stream to and from memory (what cv::FileStorage carries for detector.write / detector.read,
 * CloudProcessing.h:112,250): buf == NULL queries *size; a too small buffer is PPF_ERR_CAPACITY with *size set.
 * ppf_model_load_mem validates exactly like ppf_model_load. */
ppf_status ppf_model_save_mem(const ppf_model* m, void* buf, size_t cap, size_t* size);
ppf_status ppf_model_load_mem(const void* buf, size_t size, ppf_model** out);
/* the same validation without a device (host only): PPF_OK or PPF_ERR_IO */
ppf_status ppf_model_check_file(const char* path);

/* pcl::PPFEstimation::compute: the n x n pair features of a cloud as float32 rows of five, row i*n + j =
 * {f1, f2, f3, f4, alpha_m} of the pair (i, j) -- `feature` PPF_FEATURE_PPF: the three acos angles and the distance of the
 * reference's library; PPF_FEATURE_DARBOUX: pcl::computePairFeatures' values; alpha_m in the engine's frame convention.
 * Rows i == j and degenerate pairs are NaN.  cap_rows: rows `out` can hold (>= n*n).  Computed on the device. */
ppf_status ppf_pair_features(const float* xyzn, int n, int stride, int normal_offset, int feature, float* out, size_t cap_rows);

/* ---- matching, host buffers ------------------------------------------------------------- */
ppf_status ppf_match(const ppf_model* m, const float* scene, int ns, int sstride, int snoff, const float* edge, int ne,
                     int estride, int enoff, const ppf_match_params* params, ppf_pose* out, int cap, int* n_out);
ppf_status ppf_raw_votes(const ppf_model* m, const float* scene, int ns, int sstride, int snoff, const float* edge, int ne,
                         int estride, int enoff, const ppf_match_params* params, ppf_vote* votes, ppf_pose* raw_poses, int cap,
                         int* n_ref, ppf_match_stats* stats);

/* Many crops x many models (BASELINE config C5): every scene is uploaded and sampled once and matched against
 * every model.  out holds n_scenes x n_models blocks of `cap` poses (best first), n_out the count of each block.
 * (= ppf_batch_create(min(4, n_scenes)) + ppf_batch_run + ppf_batch_destroy) */
ppf_status ppf_match_batch(const ppf_model* const* models, int n_models, const float* const* scenes, const int* ns,
                           int sstride, int snoff, int n_scenes, const ppf_match_params* params, ppf_pose* out, int cap, int* n_out);
/* The reusable form: `lanes` HIP streams, each with its own workspace and pinned staging.  Crop c runs on lane c mod
 * lanes, its matches against all models back to back without host involvement; one synchronisation at the end.
 * scenes_on_device != 0: `scenes` are device pointers (no staging).  out / n_out / stats may be NULL. */
ppf_status ppf_batch_create(int lanes, ppf_batch** out);
ppf_status ppf_batch_destroy(ppf_batch* b);
/* record HIP events around the kernels of every match of the following runs (ppf_batch_stats.ms_*_kernel) */
ppf_status ppf_batch_enable_timing(ppf_batch* b, int on);
ppf_status ppf_batch_run(ppf_batch* b, const ppf_model* const* models, int n_models, const float* const* scenes, const int* ns,
                         int sstride, int snoff, int n_scenes, int scenes_on_device, const ppf_match_params* params, ppf_pose* out,
                         int cap, int* n_out, ppf_batch_stats* stats);
/* device block of the last run: n_scenes * n_models * cap pose records (zero rows past each count), e.g. for a gather */
ppf_status ppf_batch_device_block(ppf_batch* b, void** d_poses, int* n_records);
/* device-to-device copy of the first n_records of that block into d_dst, enqueued on `stream` */
ppf_status ppf_batch_copy_block(ppf_batch* b, void* d_dst, int n_records, void* stream);

/* ---- matching, device-resident clouds + explicit stream ---------------------------------- */
ppf_status ppf_workspace_create(ppf_workspace** out);
ppf_status ppf_workspace_destroy(ppf_workspace* ws);
/* Tuning / test knobs of a workspace.  PPF_OPT_HIT_FRACTION: expected hits per scene pair, which sizes the hit pools of
 * the next call (normally learned from the previous calls; a too small value only costs a repeat of the call).
 * PPF_OPT_GROUP_ROUND_BUCKETS: bucket ids grouped per pass over a reference point's hits (0 = as many as fit LDS). */
#define PPF_OPT_HIT_FRACTION 1
#define PPF_OPT_GROUP_ROUND_BUCKETS 2
#define PPF_OPT_CLUSTER_SERIAL 3 /* != 0: the serial greedy cluster assignment (the path for > 11,520 poses) for any size */
#define PPF_OPT_ACC32 4          /* 0 (default): 16-bit accumulator cells first, 32-bit cells for the (reference point, tile)s whose cells overflow;
                                   a workspace that sees a twentieth of a call's votes cast twice that way goes to 32-bit cells for
                                   everything; 1: 32-bit cells for everything from the first call; 2: 16-bit cells first, always;
                                   3: the (reference point, tile)s that will cast more votes than a limit learned from the previous
                                   call go straight to 32-bit cells (measured slower than 0 on BASELINE's C4: kept for the comparison) */
#define PPF_OPT_TABLE_FRACTION 5 /* expected count tables per hit (sizes the table pool of the next call; learned from then on) */
#define PPF_OPT_BATCH_REFS 6     /* > 0: at most this many reference points per batch of a call (default: what 4 GB of hit scratch hold); a test knob */
#define PPF_OPT_RUN_STAGING 7    /* > 0: the size of the vote kernel's staging area, in runs of 24 bytes (rounded down to a multiple of 64, at
                                   least 64; default: what the LDS holds next to the model's accumulator tile, 704 .. 1,024).  The area holds one 16-byte
                                   record per work item of a reference point, ((runs + 1) * 24 + 15) / 16 of them: 64 -> 98, 704 -> 1,058, 1,024 -> 1,538.
                                   A test knob: several segments per reference point on small scenes */
ppf_status ppf_workspace_set_option(ppf_workspace* ws, int option, double value);
/* record HIP events around the kernels of each call (read back through ppf_workspace_results' stats) */
ppf_status ppf_workspace_enable_timing(ppf_workspace* ws, int on);
/* Enqueue sampling + voting + pose assembly (+ clustering) on `stream` (a hipStream_t, NULL = default
 * stream).  d_scene/d_edge are DEVICE pointers.  Returns after enqueueing when everything could be
 * sized without a host round trip (presampled clouds); results stay in the workspace. */
ppf_status ppf_match_device(const ppf_model* m, ppf_workspace* ws, const float* d_scene, int ns, int sstride, int snoff,
                            const float* d_edge, int ne, int estride, int enoff, const ppf_match_params* params, void* stream);
/* Wait for the workspace's last call and copy results out (any pointer may be NULL). */
ppf_status ppf_workspace_results(ppf_workspace* ws, ppf_vote* votes, ppf_pose* raw_poses, int cap_ref, int* n_ref,
                                 ppf_pose* poses, int cap_poses, int* n_poses, ppf_match_stats* stats);
/* exact per-reference-point counters of the last call: accumulator increments and pairs hashed */
ppf_status ppf_workspace_ref_counters(ppf_workspace* ws, uint64_t* votes_per_ref, uint64_t* pairs_per_ref, int cap);
/* Full accumulators (n_ref x n_model*num_angles u32, the reference's `accumulator` array before its
 * argmax scan) of the voted reference points; presampled clouds only.  Debug / parity surface: the tests compare
 * every cell with the CPU oracle's accumulator, on every voting path (direct items and count tables, 16- and 32-bit
 * cells, the re-vote after a 16-bit overflow, several tiles, staging segments, group rounds and batches, repeated
 * calls), on scenes with planted pairs whose alpha bin is num_angles: the vote that spills into the next model
 * row's bin 0, at a tile's half boundary, at a tile boundary, and behind the last row, where it is dropped.
 * ppf_debug_accumulators runs the call on a fresh workspace (cold, default options). */
ppf_status ppf_debug_accumulators(const ppf_model* m, const float* scene, int ns, int sstride, int snoff, const float* edge, int ne,
                                  int estride, int enoff, const ppf_match_params* params, uint32_t* acc, size_t cap_words,
                                  int* n_ref);
/* The same on the caller's workspace (the host buffers go through the default stream): the call runs with the workspace's
 * options, its learned pool estimates and its 16/32-bit decision, is repeated when a pool runs out (the dump starts from
 * zeros again), and leaves its results readable through ppf_workspace_results and ppf_workspace_ref_counters. */
ppf_status ppf_debug_accumulators_ws(const ppf_model* m, ppf_workspace* ws, const float* scene, int ns, int sstride, int snoff,
                                     const float* edge, int ne, int estride, int enoff, const ppf_match_params* params, uint32_t* acc,
                                     size_t cap_words, int* n_ref);
/* Size of the cached device block a request of `bytes` is served from (host only, no device needed): classes of 1/8
 * octave, so at most 12.5 % more than asked for.  Test surface of the block cache's keying. */
size_t ppf_debug_block_size(size_t bytes);
/* How a match call is cut into batches of reference points and how big its hit pools and LDS areas are (host only, no
 * device needed): the engine's own sizing function, which a call runs once, after the cold count if there is one.  A
 * pure function of these numbers, so its corners (the worst-case single stripe, the 32,768-row grid limit, the 64-hit
 * floor, capacities near 2^32) are reached without a scene of that size.  Test surface. */
typedef struct ppf_debug_match_plan_in {
  int32_t n_ref, n_paired;   /* reference points voted by the call, rows of the paired cloud: both >= 1 */
  double hit_frac, run_frac, tbl_frac; /* expected hits per scene pair, runs per hit, count tables per hit */
  int32_t count_tables;      /* != 0: many-hit runs vote through count tables (vote_mode, alpha range and num_angles allow it) */
  int32_t batch_refs_cap, round_buckets_cap, run_seg_cap; /* PPF_OPT_BATCH_REFS, _GROUP_ROUND_BUCKETS, _RUN_STAGING; 0 = none */
  uint32_t n_buckets;        /* ppf_model_info::n_buckets, ::tile_refs, ::num_angles of the model */
  int32_t tile_refs, num_angles;
} ppf_debug_match_plan_in;
typedef struct ppf_debug_match_plan_out {
  int32_t pair_chunks;       /* pair-kernel workgroups per reference point */
  int32_t n_rounds, round_buckets; /* grouping rounds, buckets counted per round */
  int32_t batch, n_batches;  /* reference points per batch, batches of the call */
  int32_t stripe_bits;       /* log2 of the raw hit pool's stripes */
  uint32_t stripe_cap, sorted_cap, run_cap, table_cap; /* capacity of a stripe, of the sorted pool, the run table, the count-table pool */
  int32_t run_seg;           /* the vote kernel's staging area, in runs of 24 bytes */
  uint64_t vote_lds, group_lds; /* dynamic LDS of the vote and the grouping kernel, bytes */
} ppf_debug_match_plan_out;
/* PPF_ERR_INVALID for a NULL or out-of-range argument, and -- as the match call itself -- for a model tile that leaves
 * the vote kernel's least staging no LDS and for more paired points than one call can group; `out` is then all zero. */
ppf_status ppf_debug_match_plan(const ppf_debug_match_plan_in* in, ppf_debug_match_plan_out* out);
/* How one launch sequence of the batched ICP lays its jobs out in the shared scratch arrays, schedules their levels and
 * sizes its launches and its pinned block (host only, no device needed): the engine's own planning function, which
 * every ppf_icp_refine*, ppf_icp_register and ppf_match_frame call runs once per launch sequence.  A pure function of
 * the jobs' row counts and four parameters, so its corners (chunks of 64, row blocks of 8,192, steps that are no power
 * of two, the 32,768-row staging limit, rows per wave of the neighbour search) are reached without a device.  A launch
 * sequence holds up to 256 jobs and a call up to 30 levels; this record holds 8 of each, and reports the first and the
 * last job.  Test surface. */
typedef struct ppf_debug_icp_plan_in {
  int32_t n[8], nd_all[8];   /* rows of each job's source and destination cloud: all >= 1 */
  int32_t jobs;              /* 1 .. 8 */
  int32_t uniform;           /* != 0: every job has the same two clouds and the same layout (so equal n and nd_all) */
  int32_t iterations;        /* ppf_icp_params: >= 0 */
  float tolerance, rejection_scale;
  int32_t num_levels;        /* 0 .. 8 */
} ppf_debug_icp_plan_in;
typedef struct ppf_debug_icp_plan_out {
  uint64_t t_src, t_dst, t_sel, t_parts, t_sums, t_sumd; /* all jobs' rows of either cloud, selections, chunk partials, chunk sums */
  uint64_t g_start, g_cur, g_box2, g_box1u, state, bb_parts; /* elements of the arrays with a fixed pitch per job, of the states, of the extents per chunk */
  uint64_t table_bytes, levels_off;  /* both device tables, where the level table starts */
  uint64_t h_done_off, h_state_off, h_tables_off, pinned_bytes; /* the pinned block: the tick counter is at 0 */
  uint64_t first_off[8], last_off[8]; /* job 0's and the last job's o_src0, o_dst0, o_best, o_owner, o_sel, o_parts, o_sums, o_sumd */
  int32_t max_chunks, max_rows_blocks, max_dst_blocks; /* grid extents of the set-up launches */
  int32_t robust;            /* rejection_scale > 0 */
  int32_t n_levels, pad0;    /* entries used below, [level] */
  double tol_p[8];
  int64_t sum_ns[8];
  uint64_t tail_lds[8];      /* dynamic LDS of k_icp2_tail, bytes */
  int32_t max_iter[8], max_ns[8], nn_rows[8];
  uint32_t nn_blocks[8], begin_blocks[8];
  int32_t first_level[8][5], last_level[8][5]; /* job 0's and the last job's step, ns, nd, step_shift, staged */
  int32_t uni[8][7];         /* uniform: ns, nd, step, step_shift, staged, n, nd_all handed to the per-pass kernels; else 0 */
  uint64_t uni_p_sel[8], uni_p_parts[8]; /* ... and their pitches of sel and parts */
} ppf_debug_icp_plan_out;
/* PPF_ERR_INVALID for a NULL or out-of-range argument (uniform with unequal jobs included); `out` is then all zero. */
ppf_status ppf_debug_icp_plan(const ppf_debug_icp_plan_in* in, ppf_debug_icp_plan_out* out);
/* The group records ppf_model_load derives from a model's pair records (host only, no device needed): `model_bytes` is a
 * model file's byte stream, validated exactly like ppf_model_load_mem (PPF_ERR_IO).  grp_records takes records of four
 * words {row_a, row_b, cells_a, cells_b}, grp_hdr entries of two {first group record, group records}, one per 32 pair
 * records; the capacities count records and entries.  Either buffer may be NULL; the counts are always reported, and a
 * buffer that is too small is PPF_ERR_CAPACITY.  A model that votes through no count table reports 0 and 0.  Test surface. */
ppf_status ppf_debug_model_row_groups(const void* model_bytes, size_t size, uint32_t* grp_records, size_t cap_records,
                                      uint32_t* grp_hdr, size_t cap_hdr, uint64_t* n_records_out, uint64_t* n_hdr_out);
/* Guard mode of the device block cache: finds stores outside a scratch or result buffer and reads of scratch that was
 * never written, which the cache otherwise hides (a request is rounded up to a size class, so a store a few bytes too far
 * lands in slack nobody reads, and a reused block still holds the previous call's bytes).  mode 0: off (the default);
 * 1, 2: every block acquired from now on gets a 256-byte zone in front of it and a zone of at least 4 KiB right behind
 * the bytes asked for, both filled with 0xA5, and its usable bytes are filled with the 32-bit word 0 (mode 1) or 1
 * (mode 2): a result that differs between the two modes, or from the guard-off result, read memory nobody wrote.  The
 * zones are read back when a block is released and by ppf_debug_pool_check (the first 4 KiB of the back zone).  Switching
 * trims the cache; blocks already live keep the mode they were acquired in.  Sub-buffers a stage carves out of one block
 * itself have no zones between them.  PPF_POOL_GUARD=1|2 in the environment turns the mode on from the first allocation
 * and prints each violation to stderr ("ppf pool guard: ...") when it is found.  PPF_ERR_INVALID for any other mode,
 * PPF_ERR_HIP without a device.  Debug / test surface: every acquire waits for the device. */
ppf_status ppf_debug_pool_guard(int mode);
typedef struct ppf_debug_pool_violation {
  uint64_t requested_bytes; /* what the block's reserve asked for */
  int64_t first_offset;     /* of the first damaged byte from the block's usable start: < 0 in the front zone, >= requested_bytes behind */
  uint64_t n_bytes_damaged; /* in both zones together */
} ppf_debug_pool_violation;
typedef struct ppf_debug_pool_report {
  uint64_t n_blocks_live;    /* guarded blocks in use */
  uint64_t n_blocks_checked; /* the live ones, and those released since the last check */
  uint64_t n_violations;     /* damaged blocks among them */
  ppf_debug_pool_violation first[8];
} ppf_debug_pool_report;
/* Waits for the device, checks the zones of every live guarded block, adds the violations found at releases since the
 * last check and forgets those. */
ppf_status ppf_debug_pool_check(ppf_debug_pool_report* r);
/* Evaluate include/ppf_detmath.h on the device: fn 0 acos(x), 1 sin(x), 2 cos(x), 3 atan2(x, y), 4 sqrt(x),
 * 5 x / y.  The bit patterns must equal the host's (tests/test_gpu_detmath.py). */
ppf_status ppf_debug_device_math(int fn, const double* x, const double* y, double* out, int n);
/* device pointer to the per-reference pose records of the last call (n_ref x ppf_pose), for a
 * collective gather without a host copy */
ppf_status ppf_workspace_device_poses(ppf_workspace* ws, void** d_raw_poses, int* n_ref);
/* Device-side result blocks, enqueued on `stream` (call ppf_workspace_results first: it is what notices and repeats a
 * call whose hit pools were too small).  d_dst receives k (cap) ppf_pose records, zero rows past the available count:
 * the best k clustered poses / the per-reference poses.  For collectives that gather from device memory. */
ppf_status ppf_workspace_copy_top_poses(ppf_workspace* ws, void* d_dst, int k, void* stream);
ppf_status ppf_workspace_copy_raw_poses(ppf_workspace* ws, void* d_dst, int cap, void* stream);
/* clusterPoses on a DEVICE pose list (e.g. the all-gathered per-reference poses of all ranks), enqueued on `stream`;
 * the clusters are fetched with ppf_workspace_results(poses) or ppf_workspace_copy_top_poses */
ppf_status ppf_cluster_poses_device(const ppf_model* m, ppf_workspace* ws, const void* d_in, int n, int num_poses,
                                    const ppf_match_params* params, void* stream);
/* cluster a caller-supplied pose list (e.g. the all-gathered per-reference poses of all ranks) */
ppf_status ppf_cluster_poses(const ppf_model* m, const ppf_pose* in, int n, int num_poses,
                             const ppf_match_params* params, ppf_pose* out, int cap, int* n_out);

/* ---- helpers on the path's edges --------------------------------------------------------- */
/* samplePCByQuantization: returns rows through *n_out (out may be NULL to query) */
ppf_status ppf_sample_cloud(const float* xyzn, int n, int stride, int normal_offset, double relative_step, float* out, int cap_rows,
                            int* n_out);
/* out: n x 6 packed rows */
ppf_status ppf_transform_pc_pose(const float* xyzn, int n, int stride, int normal_offset, const double* pose16, float* out);


/* ---- ICP refinement of matched poses (the step right after the path) ---------------------- */
/* registerModelToScene(model, scene, poses): every pose moves the model, a multi-level point-to-plane ICP registers
 * the moved model to the scene, and the pose becomes poseICP * pose (pose/q/t/angle/residual are rewritten, votes
 * and model_index kept).  iterations_out (optional) receives the iterations spent per pose.  Host clouds. */
ppf_status ppf_icp_refine(const float* model, int n_model, int mstride, int mnoff, const float* scene, int n_scene, int sstride,
                          int snoff, const ppf_icp_params* params, ppf_pose* poses_io, int n_poses, int* iterations_out);
/* same with DEVICE-resident clouds and an explicit hipStream_t (poses_io stays on the host) */
ppf_status ppf_icp_refine_device(const float* d_model, int n_model, int mstride, int mnoff, const float* d_scene, int n_scene,
                                 int sstride, int snoff, const ppf_icp_params* params, ppf_pose* poses_io, int n_poses,
                                 int* iterations_out, void* stream);
/* registerModelToScene(src, dst, residual, pose): one registration without an initial pose */
ppf_status ppf_icp_register(const float* src, int n_src, int sstride, int snoff, const float* dst, int n_dst, int dstride, int dnoff,
                            const ppf_icp_params* params, double* pose16_out, double* residual_out, int* iterations_out);

/* ---- the producers of the N x 6 input (CloudProcessing.h:263-427), device-resident between stages ---------- */
/* cols = 3 (xyz; normals zero; normal_offset ignored) or 6 (xyz + the normal at normal_offset), `stride` floats between rows */
ppf_status ppf_cloud_upload(const float* rows, int n, int stride, int normal_offset, int cols, ppf_cloud** out);
/* the curvature ppf_cloud_upload leaves zero: n = the cloud's rows floats, copied before the call returns (what a
 * pcl::PointCloud<pcl::Normal> carries beside its normals, and what ppf_prep_regions and ppf_prep_edges read) */
ppf_status ppf_cloud_set_curvature(ppf_cloud* c, const float* curvature, int n);
ppf_status ppf_cloud_release(ppf_cloud* c);
ppf_status ppf_cloud_size(const ppf_cloud* c, int* n);
/* rows6: n x 6 floats, curvature: n floats; either may be NULL */
ppf_status ppf_cloud_download(const ppf_cloud* c, float* rows6, float* curvature, int cap_rows);
/* device pointer to the packed n x 6 rows (valid while the cloud lives): feeds ppf_match_device / ppf_icp_refine_device */
ppf_status ppf_cloud_device_rows(const ppf_cloud* c, const float** d_rows6, int* n);
/* SceneCropping (:263-339) for one box {x, y, width, height}: +-30 px, mean corner depth, corners pushed 0.15 m back,
 * points inside the pyramid {camera centre, 4 corners} are kept.  depth: HOST image (rows x cols float, metres),
 * intr = {fx, fy, ppx, ppy}. */
ppf_status ppf_prep_crop(const ppf_cloud* in, const int* box_xywh, const float* depth, int depth_rows, int depth_cols,
                         const double* intr, ppf_cloud** out);
/* Subsampling (:361-380): pcl::VoxelGrid, cubic leaf */
ppf_status ppf_prep_voxel_grid(const ppf_cloud* in, double leaf, ppf_cloud** out);
/* OutlierProcessing (:341-360): pcl::StatisticalOutlierRemoval(meanK, stddevMul) */
ppf_status ppf_prep_outlier_removal(const ppf_cloud* in, int mean_k, double stddev_mul, ppf_cloud** out);
/* NormalEstimation (:381-405): k-neighbour plane fit, normals towards the camera centre, curvature */
ppf_status ppf_prep_normals(const ppf_cloud* in, int k, ppf_cloud** out);
/* EdgeExtraction (:406-427): curvature > threshold */
ppf_status ppf_prep_edges(const ppf_cloud* in, float curvature_threshold, ppf_cloud** out);
/* PointCloudXYZNormalToMat (:163-190): rows with re-normalised normals */
ppf_status ppf_prep_to_mat(const ppf_cloud* in, ppf_cloud** out);
/* match / match_S2B (:442, :495) and the ICP step (:465-470, :518-523) on clouds that are already resident (the
 * outputs of ppf_prep_to_mat): crop -> ... -> edges -> match -> ICP without a host copy of any cloud */
ppf_status ppf_match_clouds(const ppf_model* m, const ppf_cloud* scene, const ppf_cloud* edge, const ppf_match_params* params,
                            ppf_pose* out, int cap, int* n_out);
ppf_status ppf_icp_refine_clouds(const ppf_cloud* model, const ppf_cloud* scene, const ppf_icp_params* params, ppf_pose* poses_io,
                                 int n_poses, int* iterations_out);
/* exact neighbour lists (parity surface): idx, d2 are [n][k], ascending (distance, index) */
ppf_status ppf_prep_knn(const ppf_cloud* in, int k, int* idx, float* d2);

/* ---- support planes: the table or wall the objects stand on, found and taken out of a cloud --------- */
#define PPF_PLANE_NONE 0     /* round not run: fewer than 3 rows left, or an earlier round ended the search */
#define PPF_PLANE_REMOVED 1
#define PPF_PLANE_REJECTED 2 /* best hypothesis below min_inliers / min_inlier_share: nothing removed, search ends */
#define PPF_PLANE_NO_REFIT 1      /* flags: remove the best hypothesis as it is */
#define PPF_PLANE_REMOVE_BEHIND 2 /* flags: also remove rows farther than the threshold on the side away from the origin */
#define PPF_PLANE_MAX_PLANES 4
#define PPF_PLANE_MAX_HYPOTHESES 4096

typedef struct ppf_plane_params {
  float distance_threshold; /* > 0, metres; default 0.005 */
  int32_t n_hypotheses;     /* 1..4096; default 256 */
  uint32_t seed;            /* default 1 */
  int32_t max_planes;       /* 1..4; default 1 */
  int32_t min_inliers;      /* >= 3; default 100 */
  float min_inlier_share;   /* 0..1, of the rows left at the round's start; default 0.10 */
  int32_t flags;
  int32_t reserved[4];
} ppf_plane_params;

typedef struct ppf_plane_info {
  double n[3], d;        /* n.p + d = 0, |n| = 1, d >= 0: the origin (the camera) is on the non-negative side */
  int32_t status;        /* PPF_PLANE_* */
  int32_t hypothesis;    /* the index of the best hypothesis */
  int32_t n_rows;        /* rows left at the round's start */
  int32_t n_hyp_inliers; /* inliers of the best hypothesis */
  int32_t n_inliers;     /* inliers of the plane that was removed */
  int32_t n_behind;      /* rows removed as behind it (PPF_PLANE_REMOVE_BEHIND) */
  int32_t refit;         /* 1: n, d are the refitted plane, 0: the hypothesis */
  int32_t reserved;
} ppf_plane_info;

typedef struct ppf_plane_stats {
  int32_t n_clouds, n_launches, n_host_syncs;
  float ms_wall;
  int32_t reserved[4];
} ppf_plane_stats;

void ppf_default_plane_params(ppf_plane_params* p);
/* Up to max_planes rounds per cloud, n_clouds (0..256) clouds in one pass: a round draws n_hypotheses planes through three
 * of the rows left (a hash of seed, round, hypothesis: the same rows on every machine), counts each one's inliers
 * (|n.p + d| <= distance_threshold in fp64), refits the best by the fixed-order covariance of its inliers (unless
 * PPF_PLANE_NO_REFIT; the refit is used iff it counts no fewer inliers) and removes that plane's inliers.  out[i]: the kept
 * rows of in[i] in their order, normals and curvature carried byte for byte; the outputs share one device block.
 * info: [n_clouds][max_planes] rows, zero for a round that did not run.  labels: NULL, or n_clouds pointers each NULL or
 * rows(in[i]) bytes: 0 kept, 1 + p inlier of plane p, 0x80 | (1 + p) removed as behind plane p.  A non-finite row is never
 * removed.  Each cloud's result is what a call with that cloud alone gives; the launch count depends on max_planes and flags
 * only; the host blocks in one upload before any device work and waits for the device once, for the results (n_host_syncs 1).  Argument errors are PPF_ERR_INVALID before any device work; on every
 * error each out[i] is NULL and the info rows are zero. */
ppf_status ppf_prep_planes(const ppf_cloud* const* in, int n_clouds, const ppf_plane_params* p, ppf_cloud** out,
                           ppf_plane_info* info, uint8_t* const* labels, ppf_plane_stats* stats /* may be NULL */);
/* The rows of a companion cloud (a detection's edge cloud) that are neither inliers of one of the n_planes (0..4) planes
 * whose status is PPF_PLANE_REMOVED nor, with PPF_PLANE_REMOVE_BEHIND, behind one: the same predicate and
 * distance_threshold.  Applied to in[i] itself it gives out[i]. */
ppf_status ppf_prep_planes_apply(const ppf_cloud* in, const ppf_plane_info* planes, int n_planes, const ppf_plane_params* p,
                                 ppf_cloud** out);

/* ---- object clusters: a plane-free cloud split into its connected blobs ------------------------------ */
#define PPF_CLUSTER_MAX_CLUSTERS 256 /* what ppf_prep_frame takes as boxes */

typedef struct ppf_cluster_params {
  float tolerance;      /* > 0, metres; default 0.02 */
  int32_t min_size;     /* >= 1; default 100 */
  int32_t max_size;     /* 0: no bound; default 0 */
  int32_t max_clusters; /* 1..256; default 64 */
  int32_t flags;        /* none defined: 0 */
  int32_t reserved[4];
} ppf_cluster_params;

typedef struct ppf_cluster_info {
  int32_t n_rows;
  int32_t first_row;   /* the cluster's smallest row index in its cloud */
  float lo[3], hi[3];  /* the minimum and maximum of its rows */
  int32_t box_xywh[4]; /* its image box {umin, vmin, umax - umin, vmax - vmin}; zero without intrinsics or without a row of z > 0 */
  int32_t reserved[4];
} ppf_cluster_info;

typedef struct ppf_cluster_stats {
  int32_t n_clouds, n_launches, n_host_syncs;
  float ms_wall;
  int32_t reserved[4];
} ppf_cluster_stats;

void ppf_default_cluster_params(ppf_cluster_params* p);
/* Euclidean cluster extraction (pcl::EuclideanClusterExtraction) of n_clouds (0..256) clouds in one pass.  A row is finite iff
 * x, y, z are; finite rows a, b are linked iff ((dx*dx + dy*dy) + dz*dz) <= (double)tolerance * (double)tolerance with
 * dx = (double)ax - (double)bx ..., all in fp64; a component is a connected component of the links, first_row its smallest
 * row index; it is valid iff min_size <= n_rows and (max_size == 0 or n_rows <= max_size); the valid components ranked by
 * n_rows descending, then first_row ascending, the first min(valid, max_clusters) of them are the cloud's clusters.
 * out: [n_clouds][max_clusters] clouds, a cluster's rows in ascending row index with normals and curvature carried byte for
 * byte, NULL past the cloud's cluster count; they are views into one device block and are released in any order.
 * info: [n_clouds][max_clusters], zero past the count.  With intr = {fx, fy, ppx, ppy} the image box of a cluster spans
 * u = (int)floor((((double)x / (double)z) * fx + ppx) + 0.5), v likewise, clipped to the image, of its rows with z > 0;
 * intr == NULL: the boxes are zero and image_rows / image_cols are ignored.  counts: [n_clouds][3] = {clusters output, valid
 * components, all components}.  labels: NULL, or n_clouds pointers each NULL or rows(in[i]) int32: the rank of the row's
 * cluster, or -1.  Each cloud's result is what a call with that cloud alone gives.  The launch count depends on nothing but
 * whether any cloud has a row; the host blocks in one upload before any device work and waits for the device once
 * (n_host_syncs 1).  A cloud whose finite extent needs more than 1,024 grid cells of 0.5773 * tolerance on an axis is
 * PPF_ERR_INVALID (the message names the smallest tolerance that fits).  Argument errors are PPF_ERR_INVALID before any device
 * work; on every error each out is NULL and info and counts are zero. */
ppf_status ppf_prep_clusters(const ppf_cloud* const* in, int n_clouds, const ppf_cluster_params* p, const double* intr /* may be NULL */,
                             int image_rows, int image_cols, ppf_cloud** out, ppf_cluster_info* info, int32_t* counts,
                             int32_t* const* labels, ppf_cluster_stats* stats /* may be NULL */);

/* ---- smooth surface regions: what cuts objects that touch, where distance alone cannot -------------- */
#define PPF_REGION_UNORIENTED 1 /* flags: normals agree on |dot| (pcl::RegionGrowing's rule, for normals of no common orientation) */

typedef struct ppf_region_params {
  float tolerance;           /* > 0, metres; default 0.01 */
  float normal_cos;          /* finite, -1..1; default 0.9659258f (15 degrees) */
  float curvature_threshold; /* >= 0, +inf allowed (every eligible row smooth), not NaN; default 0.03, the project's edge cut */
  int32_t min_size;          /* >= 1; default 100 */
  int32_t max_size;          /* 0: no bound */
  int32_t max_regions;       /* 1..256; default 64 */
  int32_t flags;             /* 0 | PPF_REGION_UNORIENTED */
  int32_t reserved[4];
} ppf_region_params;

void ppf_default_region_params(ppf_region_params* p);
/* Region growing on normals, as a closed specification, of n_clouds (0..256) clouds in one pass.  Normals are taken as they
 * are.  A row is eligible iff x, y, z, nx, ny, nz are finite (every other row belongs to no region), smooth iff it is eligible
 * and curvature <= curvature_threshold (a float comparison: a NaN curvature is not smooth), a border row iff eligible and
 * not smooth.  near(a, b) iff ((dx*dx + dy*dy) + dz*dz) <= (double)tolerance * (double)tolerance as in ppf_prep_clusters;
 * agree(a, b) iff dot >= (double)normal_cos with dot = ((double)anx*(double)bnx + (double)any*(double)bny) +
 * (double)anz*(double)bnz (fabs(dot) with PPF_REGION_UNORIENTED), all in fp64.  Two smooth rows are linked iff near and agree;
 * a component is a connected component of the links over a cloud's smooth rows.  A border row joins the component of the
 * smooth row with the smallest squared distance (ties: the smaller row index) among those it is near to and agrees with, or
 * no region; border rows link nothing.  n_rows counts a component's smooth and attached border rows; from there on validity,
 * ranking, out, info, labels, the image boxes and the grid limit (over the eligible rows) are ppf_prep_clusters', with
 * max_regions for max_clusters -- except that a region's info.first_row is its smallest SMOOTH row.  counts: [n_clouds][4] =
 * {regions output, valid components, all components, border rows attached}.  Each cloud's result is what a call with that
 * cloud alone gives; the launch count depends on nothing but whether any cloud has a row; one upload before any device work
 * and one wait (n_host_syncs 1).  Argument errors are PPF_ERR_INVALID before any device work; on every error each out is
 * NULL and info and counts are zero. */
ppf_status ppf_prep_regions(const ppf_cloud* const* in, int n_clouds, const ppf_region_params* p, const double* intr /* may be NULL */,
                            int image_rows, int image_cols, ppf_cloud** out, ppf_cluster_info* info, int32_t* counts,
                            int32_t* const* labels, ppf_cluster_stats* stats /* may be NULL */);

/* ---- the organised scene cloud from a depth image, on the device (what CloudProcessor::Deprojection leaves empty) -- */
#define PPF_DEPTH_F32 0  /* float32 metres: z = value (the reference's EXR frame) */
#define PPF_DEPTH_U16 1  /* uint16 sensor units: z = (float)((double)d * depth_scale) (Azure Kinect, RealSense) */
#define PPF_DEPTH_FP64 1 /* flags bit: x = (float)(((double)u - ppx) * (double)z / fx) in fp64 instead of Camera::back_projection's
                            x = (float)((double)((float)((double)u - ppx) * z) / fx); y likewise with v, ppy, fy */
typedef struct ppf_depth_params {
  int32_t format;     /* PPF_DEPTH_F32 | PPF_DEPTH_U16 */
  int32_t flags;      /* 0 | PPF_DEPTH_FP64 */
  double depth_scale; /* U16: metres per unit, > 0; ignored for F32 */
  float z_min, z_max; /* a pixel is kept iff z is finite, z > 0, z >= z_min and (z_max == 0 or z <= z_max); z_max 0: no upper bound */
  int32_t reserved[4];
} ppf_depth_params;
/* PPF_DEPTH_F32, flags 0, depth_scale 0.001, z_min 0, z_max 0 */
void ppf_default_depth_params(ppf_depth_params* p);
/* Back-project every kept pixel of a rows x cols depth image, intr = {fx, fy, ppx, ppy} as ppf_prep_crop takes it.  The
 * rows of *out are x y z 0 0 0 (curvature 0) in row-major pixel order (v, then u: the order of np.nonzero(depth > 0)),
 * byte-identical to ppf_cloud_upload of the same xyz with cols = 3; an image without a kept pixel gives an empty cloud.
 * depth: HOST image whose rows are row_pitch_bytes apart (0: packed).  Argument errors (NULL pointers, rows or cols
 * <= 0, rows * cols > INT32_MAX, a pitch below cols * element size or not a multiple of it, a misaligned image, an
 * unknown format or flag, a U16 scale <= 0, fx or fy zero or not finite, ppx, ppy, z_min or z_max not finite, z_max < 0)
 * are PPF_ERR_INVALID before any device work; on any error *out is NULL. */
ppf_status ppf_cloud_from_depth(const void* depth, int rows, int cols, size_t row_pitch_bytes, const double* intr,
                                const ppf_depth_params* p, ppf_cloud** out);
/* the same from DEVICE memory: the work is enqueued on `stream` (a hipStream_t, NULL: default stream) and the call returns
 * when the cloud is complete.  A pointer the current device cannot read, or an image that runs past the end of its
 * allocation, is PPF_ERR_INVALID before anything is launched. */
ppf_status ppf_cloud_from_depth_device(const void* d_depth, int rows, int cols, size_t row_pitch_bytes, const double* intr,
                                       const ppf_depth_params* p, void* stream, ppf_cloud** out);

/* ---- the same cloud with normals and curvature from the image's own neighbourhoods ----------------- */
#define PPF_DEPTH_NORMALS_DROP 1 /* flags: rows without a normal are left out of the cloud */
#define PPF_DEPTH_NORMALS_MAX_RADIUS 8
typedef struct ppf_depth_normal_params {
  int32_t radius;         /* 1..8: the window is (2r+1) x (2r+1) pixels; default 3 */
  float max_depth_change; /* finite, > 0, relative to the pixel's own z; default 0.02 */
  int32_t min_neighbours; /* 3..(2r+1)^2, the pixel itself counts; default 3 */
  int32_t flags;          /* 0 | PPF_DEPTH_NORMALS_DROP */
  int32_t reserved[4];
} ppf_depth_normal_params;
/* radius 3, max_depth_change 0.02, min_neighbours 3, flags 0 */
void ppf_default_depth_normal_params(ppf_depth_normal_params* p);
/* ppf_cloud_from_depth with a plane fit per kept pixel p = (u, v) over its image window.  q = (u + du, v + dv) is a
 * neighbour of p iff |du|, |dv| <= radius, q lies inside the image, q is kept by the same rule as p (p's formats, scale,
 * z_min, z_max) and fabs((double)zq - (double)zp) <= (double)max_depth_change * (double)zp; p is its own neighbour, k counts
 * them, and they are visited with dv ascending and du ascending inside a row.  The fit is ppf_prep_normals' over that list,
 * on the float x y z the cloud's rows hold: fp64 centroid (sequential sums, / k), in a second pass the six covariance
 * sums of q - c (/ k), the eigenvector of the smallest eigenvalue by the same 12 Jacobi sweeps, turned towards the origin
 * (flipped when -(p . n) < 0) and cast to float; curvature = (float)(|lambda| / |trace|), 0 when the trace is 0.  A pixel
 * with k < min_neighbours gets normal NaN NaN NaN and curvature NaN, or with PPF_DEPTH_NORMALS_DROP no row (the flag never
 * changes who is a neighbour).  Without the flag the rows, their order and their xyz bytes are ppf_cloud_from_depth's of
 * the same arguments.  Everything ppf_cloud_from_depth says about depth, the pitch, intr, p, errors and *out holds; np
 * NULL, a radius outside 1..PPF_DEPTH_NORMALS_MAX_RADIUS, a max_depth_change that is not finite or <= 0, min_neighbours
 * outside 3..(2r+1)^2 or an unknown flag are PPF_ERR_INVALID before any device work too. */
ppf_status ppf_cloud_from_depth_normals(const void* depth, int rows, int cols, size_t row_pitch_bytes, const double* intr,
                                        const ppf_depth_params* p, const ppf_depth_normal_params* np, ppf_cloud** out);
/* the same from DEVICE memory on `stream`, as ppf_cloud_from_depth_device */
ppf_status ppf_cloud_from_depth_normals_device(const void* d_depth, int rows, int cols, size_t row_pitch_bytes, const double* intr,
                                               const ppf_depth_params* p, const ppf_depth_normal_params* np, void* stream,
                                               ppf_cloud** out);

/* ---- edge-preserving smoothing of the depth image itself, in front of the calls above --------------- */
#define PPF_DEPTH_FILTER_MAX_RADIUS 8
typedef struct ppf_depth_filter_params {
  int32_t radius;       /* 0..8: the window is (2r+1)^2; 0: the support test only; default 3 */
  float range_abs;      /* finite, > 0, metres; default 0.01 */
  float range_quad;     /* finite, >= 0, 1/metres: the range grows by range_quad * z^2; default 0 */
  float support_abs;    /* finite, >= 0; default 0.01 */
  float support_quad;   /* finite, >= 0; default 0 */
  int32_t min_support;  /* 0..8; 0: every kept pixel is supported; default 6 */
  int32_t flags;        /* none defined: 0 */
  int32_t reserved[4];
} ppf_depth_filter_params;
typedef struct ppf_depth_filter_stats {
  int32_t n_kept, n_unsupported, n_written; /* n_kept = n_unsupported + n_written */
  int32_t n_launches;   /* kernel launches of the call: 1 */
  int32_t n_host_syncs; /* blocking waits of the call: 1 */
  float ms_wall;
  int32_t reserved[4];
} ppf_depth_filter_stats;
/* radius 3, range_abs 0.01, range_quad 0, support_abs 0.01, support_quad 0, min_support 6, flags 0 */
void ppf_default_depth_filter_params(ppf_depth_filter_params* p);
/* Removes the unsupported ("flying") pixels of a depth image and smooths the others without crossing a depth step.  Every
 * operation is fp64 as written, nothing fused; z(p) and "kept" are ppf_cloud_from_depth's, Z = (double)z.
 *  1. Support.  S(p) = (double)support_abs + (double)support_quad * (Zp * Zp).  Of the 8 neighbours q of a kept p, one outside
 *     the image supports p (the border is no depth edge) and one inside supports p iff it is kept and
 *     fabs(Zq - Zp) <= S(p).  p is supported iff it is kept and (min_support == 0 or the count is >= min_support).  A kept
 *     pixel that is not supported counts in n_unsupported, is written as 0 and takes no part in step 2 for any pixel.
 *  2. Smoothing of a supported p.  R = (double)range_abs + (double)range_quad * (Zp * Zp), D = (double)((radius + 1) *
 *     (radius + 1)), num = den = 0.  For dv = -r..r ascending and du = -r..r ascending inside each row, q = (u + du, v + dv):
 *     skip q unless it is inside the image and supported; s = 1.0 - (double)(du*du + dv*dv) / D, skip unless s > 0;
 *     t = (Zq - Zp) / R, k = 1.0 - t * t, skip unless k > 0; w = (s * s) * (k * k); num = num + w * Zq; den = den + w.
 *     out(p) = (float)(num / den).  The centre weighs 1, so den >= 1; with radius 0 the result is z(p) exactly.
 * Both weights are Tukey biweights: a neighbour at or beyond R in depth weighs exactly 0, so a depth step stays byte for
 * byte.  out: float32 metres, packed rows x cols, 0.0f at every pixel that is not written: what ppf_cloud_from_depth*,
 * ppf_depth_register and the frame stages take as PPF_DEPTH_F32.  depth, rows, cols, row_pitch_bytes and dp (format,
 * depth_scale, z_min, z_max) are ppf_cloud_from_depth's with their errors; dp->flags is ignored.  fp NULL, a field outside
 * the range stated beside it, a non-zero flag or out NULL are PPF_ERR_INVALID before any device work too; without a device
 * the call is PPF_ERR_HIP.  One launch and one blocking wait whatever the image holds.  On any error *stats is zero and
 * out is not touched.  stats may be NULL. */
ppf_status ppf_depth_filter(const void* depth, int rows, int cols, size_t row_pitch_bytes, const ppf_depth_params* dp,
                            const ppf_depth_filter_params* fp, float* out, ppf_depth_filter_stats* stats /* may be NULL */);
/* the same between DEVICE buffers, as ppf_depth_register_device: enqueued on `stream` (a hipStream_t, NULL: default stream),
 * returns when the image is complete.  A pointer the current device cannot read, a buffer that runs past the end of its
 * allocation, or d_out overlapping the depth image is PPF_ERR_INVALID before anything is launched. */
ppf_status ppf_depth_filter_device(const void* d_depth, int rows, int cols, size_t row_pitch_bytes, const ppf_depth_params* dp,
                                   const ppf_depth_filter_params* fp, float* d_out, void* stream, ppf_depth_filter_stats* stats);

/* ---- the last frames of a fixed camera fused into one depth image: noise, holes and flicker ---------- */
#define PPF_HISTORY_MEAN 1        /* flags: the mean of the consensus instead of its lower median */
#define PPF_HISTORY_MAX_WINDOW 16
#define PPF_HISTORY_MAX_AGE 15
#define PPF_HISTORY_MEASURED 1    /* state values: the newest frame has the pixel */
#define PPF_HISTORY_FILLED 2      /*   an older frame fills the hole */
#define PPF_HISTORY_UNSUPPORTED 3 /*   fewer than min_support frames agree with the anchor */
#define PPF_HISTORY_CHANGED 16    /* state bit, on top of PPF_HISTORY_MEASURED: the newest sample agrees with nothing remembered */
typedef struct ppf_depth_history_params {
  int32_t window;      /* K, 1..16: the frames remembered, the pushed one included; default 8 */
  float range_abs;     /* finite, > 0, metres; default 0.01 */
  float range_quad;    /* finite, >= 0, 1/metres: the range grows by range_quad * z^2; default 0 */
  int32_t min_support; /* 1..window; default 1 */
  int32_t max_age;     /* 0..15: how old a sample may be and still fill a hole; 0: no hole filling; default 7 */
  int32_t flags;       /* 0 | PPF_HISTORY_MEAN */
  int32_t reserved[4];
} ppf_depth_history_params;
typedef struct ppf_depth_history_stats {
  int32_t n_kept;                                       /* kept pixels of the pushed frame */
  int32_t n_measured, n_filled, n_unsupported, n_empty; /* pixels per state: they add up to rows * cols */
  int32_t n_changed;                                    /* measured pixels with PPF_HISTORY_CHANGED */
  int64_t frame;                                        /* t of this push: pushes before it since creation or the last reset */
  int32_t n_launches;                                   /* kernel launches of the call: 1 */
  int32_t n_host_syncs;                                 /* blocking waits of the call: 1 */
  float ms_wall;
  int32_t reserved[4];
} ppf_depth_history_stats;
typedef struct ppf_depth_history_desc {
  int32_t rows, cols, window;
  int32_t reserved0;
  int64_t frames;        /* pushes since creation or the last reset */
  uint64_t device_bytes; /* device memory the handle holds: the ring and its counters */
  int32_t reserved[4];
} ppf_depth_history_desc;
typedef struct ppf_depth_history ppf_depth_history;
/* window 8, range_abs 0.01, range_quad 0, min_support 1, max_age 7, flags 0 */
void ppf_default_depth_history_params(ppf_depth_history_params* p);
/* A ppf_depth_history keeps the last K = window depth images of one camera on the device and turns every pushed frame into
 * one fused image.  It is made for one image size, one ppf_depth_params (format, depth_scale, z_min, z_max; flags is ignored)
 * and one ppf_depth_history_params.  Every operation is fp64 as written, nothing fused; z(p) and "kept" are
 * ppf_cloud_from_depth's.  Let t be the number of pushes since creation or the last reset -- the pushed frame is frame t --
 * and n_hist = min(t + 1, K).  Per pixel, s_a for the age a = 0 .. n_hist - 1 is the float z of frame t - a where that frame
 * kept the pixel, and "none" elsewhere.
 *  1. Anchor.  a* is the smallest a in 0 .. min(max_age, n_hist - 1) with s_a kept.  None: out = 0, state = 0 (empty).
 *  2. Consensus.  Za = (double)s_a*, R = (double)range_abs + (double)range_quad * (Za * Za),
 *     C = {a in 0 .. n_hist - 1 : s_a kept and fabs((double)s_a - Za) <= R}, n = |C| >= 1.
 *  3. Support.  n < min_support: out = 0, state = PPF_HISTORY_UNSUPPORTED.
 *  4. Value.  Without PPF_HISTORY_MEAN the element of rank (n - 1) / 2 (integer division: the lower median) of C's values in
 *     ascending order -- a kept value is finite and > 0, so equal values have equal bytes and no tie rule is needed; no
 *     arithmetic touches the value.  With it: sum = 0.0; for a = n_hist - 1 down to 0 (oldest first), a in C:
 *     sum = sum + (double)s_a; out = (float)(sum / (double)n).
 *  5. State.  PPF_HISTORY_MEASURED when a* = 0, PPF_HISTORY_FILLED when a* > 0.  When a* = 0, n = 1 and some older s_a is
 *     kept, PPF_HISTORY_CHANGED is OR-ed in: the newest sample disagrees with everything remembered.
 * With a* = 0 the consensus is taken around the newest sample: a surface that moved is followed in the frame it moves and
 * nothing ghosts.  With window 1 the output is the kept pixels of the input, byte for byte.
 * rows, cols and dp are ppf_cloud_from_depth's with their errors; dp or hp NULL, a field outside the range stated beside it,
 * an unknown flag or out NULL are PPF_ERR_INVALID before any device work; without a device the call is PPF_ERR_HIP; a ring
 * (window x rows x cols floats, rows padded to four pixels) that cannot be allocated is PPF_ERR_NOMEM.  On any error *out is
 * NULL. */
ppf_status ppf_depth_history_create(int rows, int cols, const ppf_depth_params* dp, const ppf_depth_history_params* hp,
                                    ppf_depth_history** out);
/* Push one frame: a HOST image of the history's size and format whose rows are row_pitch_bytes apart (0: packed), with the
 * pointer, pitch and alignment rules of ppf_cloud_from_depth.  out: float32 metres, packed rows x cols, 0.0f where nothing is
 * written: what ppf_depth_filter, ppf_cloud_from_depth*, ppf_depth_register and the frame stages take as PPF_DEPTH_F32.
 * state: packed rows x cols uint8, or NULL.  One launch and one blocking wait whatever the image and the history hold.  A
 * NULL handle, image or out, or a bad pitch, is PPF_ERR_INVALID before any device work.  On any error *stats is zero, out and
 * state are not touched and t does not advance.  Pushes on one history are serialised inside the library; different
 * histories may be pushed from different threads. */
ppf_status ppf_depth_history_push(ppf_depth_history* h, const void* depth, size_t row_pitch_bytes, float* out,
                                  uint8_t* state /* may be NULL */, ppf_depth_history_stats* stats /* may be NULL */);
/* the same between DEVICE buffers, as ppf_depth_filter_device: enqueued on `stream` (a hipStream_t, NULL: default stream),
 * returns when the image is complete.  A pointer the current device cannot read, a buffer that runs past the end of its
 * allocation, or an output overlapping the depth image or the other output is PPF_ERR_INVALID before anything is launched. */
ppf_status ppf_depth_history_push_device(ppf_depth_history* h, const void* d_depth, size_t row_pitch_bytes, float* d_out,
                                         uint8_t* d_state /* may be NULL */, void* stream,
                                         ppf_depth_history_stats* stats /* may be NULL */);
/* t back to 0: the next push sees no older frame.  The ring is not cleared, n_hist bounds what is read. */
ppf_status ppf_depth_history_reset(ppf_depth_history* h);
/* the size, the window, the pushes since the last reset and the device memory held */
ppf_status ppf_depth_history_info(const ppf_depth_history* h, ppf_depth_history_desc* info);
ppf_status ppf_depth_history_release(ppf_depth_history* h);

/* ---- the camera's motion between two depth images: whole-image projective point-to-plane ICP --------- */
#define PPF_MOTION_MAX_LEVELS 4
#define PPF_MOTION_MAX_ITERS 64
#define PPF_MOTION_NONE 0       /* level not reached: an earlier level ended the call, or l >= levels; the row is zero */
#define PPF_MOTION_CONVERGED 1  /* the last step was below eps_rot and eps_trans */
#define PPF_MOTION_MAX_ITERS_REACHED 2 /* iters[l] steps were applied */
#define PPF_MOTION_LOST 3       /* too few pairs at an evaluation: the call ends with the pose of that evaluation */
#define PPF_MOTION_STEP 4       /* a step over the limits, not finite or not solvable was refused: likewise */
#define PPF_MOTION_SKIPPED 5    /* iters[l] == 0 or n_source < min_pairs: the pose passes through to the next finer level */
typedef struct ppf_depth_motion_params {
  int32_t levels;         /* 1..4: the image must have at least one row and column at level levels - 1; default 3 */
  int32_t iters[4];       /* per level, level 0 (full size) first, each 0..64; default 10, 5, 4, 4 */
  float pyr_gate;         /* finite, > 0, metres; default 0.03 */
  float normal_gate;      /* finite, > 0, metres at level 0, doubled per level; default 0.01 */
  float dist_gate;        /* finite, > 0, metres; default 0.05 */
  float normal_cos;       /* finite, -1..1; default 0.8 */
  float max_step_rot;     /* rad, finite, > 0; default 0.3 */
  float max_step_trans;   /* metres, finite, > 0; default 0.15 */
  float eps_rot, eps_trans; /* finite, >= 0; default 1e-5 */
  float min_pair_share;   /* 0..1: pairs needed as a share of n_source; default 0.25 */
  int32_t min_pairs;      /* >= 6; default 16 */
  int32_t flags;          /* 0 */
  int32_t reserved[4];
} ppf_depth_motion_params;
typedef struct ppf_depth_motion_level {
  int32_t status, iterations;        /* PPF_MOTION_*; steps applied at this level */
  int32_t rows, cols;                /* the level's size */
  int32_t n_source;                  /* pixels of `prev` with a normal at this level */
  int32_t n_pairs_first, n_pairs_last;
  float rmse_first, rmse_last;       /* point-to-plane rms of the level's first / last evaluation, metres */
  int32_t reserved[3];
} ppf_depth_motion_level;
typedef struct ppf_depth_motion_stats {
  int32_t status;         /* the status of the last level reached */
  int32_t n_evaluations;  /* evaluations that ran, over all levels */
  int32_t n_enqueued;     /* evaluations enqueued: the sum of iters[0 .. levels - 1]; the rest returned at the state word */
  int32_t n_launches;     /* kernel launches of the call: a function of levels, iters and the image size alone */
  int32_t n_host_syncs;   /* blocking waits of the call: 1 */
  float ms_wall;
  int32_t reserved[4];
} ppf_depth_motion_stats;
/* levels 3, iters 10 5 4 4, pyr_gate 0.03, normal_gate 0.01, dist_gate 0.05, normal_cos 0.8, max_step_rot 0.3,
 * max_step_trans 0.15, eps_rot 1e-5, eps_trans 1e-5, min_pair_share 0.25, min_pairs 16, flags 0 */
void ppf_default_depth_motion_params(ppf_depth_motion_params* p);
/* The rigid motion T between two depth images of one camera: p_cur = T p_prev for a static point, so a pose (model -> camera)
 * of the previous frame is T * pose in the current one.  A projective point-to-plane ICP over a small pyramid.  Everything
 * is fp64 unless stated, evaluated as written, left to right, nothing fused; z(p) and "kept" are ppf_cloud_from_depth's.
 *  1. Level 0 of each image: the float z of a kept pixel, 0 elsewhere.
 *  2. Level l + 1 is rows_l / 2 by cols_l / 2 (integer division: an odd last row or column is dropped).  Pixel (u, v) reads the
 *     level-l pixels (2u, 2v), (2u+1, 2v), (2u, 2v+1), (2u+1, 2v+1); a value is kept when it is > 0; m is the smallest kept
 *     one; the result is the fp64 sum, in that order, of the kept values s with (double)s - (double)m <= (double)pyr_gate,
 *     divided by their count and cast to float; 0 when none is kept.  fx_{l+1} = fx_l / 2, fy likewise,
 *     ppx_{l+1} = (ppx_l - 0.5) / 2, ppy likewise.
 *  3. Maps, per level and image.  V(u, v) = (((double)u - ppx) * Z / fx, ((double)v - ppy) * Z / fy, Z), Z = (double)z.  A pixel
 *     has a normal when it and its four 4-neighbours are inside the image and kept, each neighbour's Z differs from its own by
 *     at most (double)normal_gate * 2^l, and with dx = V(u+1, v) - V(u-1, v), dy = V(u, v+1) - V(u, v-1), c = dy x dx
 *     (c0 = dy1 dx2 - dy2 dx1, c1 = dy2 dx0 - dy0 dx2, c2 = dy0 dx1 - dy1 dx0), len = sqrt((c0 c0 + c1 c1) + c2 c2) > 0,
 *     n = (float)(c_i / len) is not all zero and faces the camera: ((double)n0 V0 + (double)n1 V1) + (double)n2 V2 < 0.
 *     Nothing is flipped.
 *  4. Levels run from levels - 1 down to 0 on one T, which starts as init16 (NULL: the identity).  The source pixels of a level
 *     are the pixels of `prev` with a normal, n_source of them; the targets are those of `cur`.  A level with iters[l] == 0 or
 *     n_source < min_pairs is SKIPPED.
 *  5. Evaluation k = 0, 1, ... of a level, per source pixel (u, v) with vertex V and normal n: p_r = ((T[r][0] V0 + T[r][1] V1) +
 *     T[r][2] V2) + T[r][3], n'_r = (T[r][0] n0 + T[r][1] n1) + T[r][2] n2; p2 > 0; ui = floor((p0 * fx / p2 + ppx) + 0.5), vi
 *     likewise with fy, ppy; both inside the level's image; the pixel (ui, vi) of `cur` has a normal nt and the vertex q;
 *     dq = q - p; it is a pair when (dq0 dq0 + dq1 dq1) + dq2 dq2 <= (double)dist_gate * (double)dist_gate and
 *     (n'0 nt0 + n'1 nt1) + n'2 nt2 >= (double)normal_cos.  r = (nt0 dq0 + nt1 dq1) + nt2 dq2,
 *     J = (p1 nt2 - p2 nt1, p2 nt0 - p0 nt2, p0 nt1 - p1 nt0, nt0, nt1, nt2): the rotation is about the camera origin.
 *  6. The 28 sums of ppf_refine_frame (J_i J_j for i <= j row by row, J_i r, r r), each product rounded, then summed by a
 *     fixed tree: source pixel j = v * cols_l + u is lane j % 64 of chunk j / 64, a lane that is no pair or past the last
 *     pixel holds +0.0, a chunk is summed by lane l adding lane l + 32, then + 16, 8, 4, 2, 1; the chunk sums are reduced by
 *     the same tree, chunk c being lane c % 64 of group c / 64, and so on until one value is left.  n_pairs is an integer;
 *     rmse = (float)sqrt(sum r r / (double)n_pairs), 0 without pairs.
 *  7. LOST when n_pairs < min_pairs or (double)n_pairs < (double)min_pair_share * (double)n_source.  Otherwise the damped solve
 *     of ppf_refine_frame (A + 1e-10 trace I, first largest pivot) gives x; STEP when it fails, a component is not finite,
 *     (x0 x0 + x1 x1) + x2 x2 > max_step_rot^2 or (x3 x3 + x4 x4) + x5 x5 > max_step_trans^2 (the limits as (double) of the
 *     float, squared).  Else R = Rz(x2) Ry(x1) Rx(x0), M = [R | x3 x4 x5], T <- M T (each element the sum 0 + a0 b0 + a1 b1 +
 *     a2 b2 + a3 b3), iterations = k + 1; CONVERGED when both squares are <= eps^2, else MAX_ITERS_REACHED at
 *     k + 1 == iters[l]; both go on to the next finer level.  LOST and STEP end the call with the pose of the evaluation that
 *     raised them; the finer levels stay NONE, their rows zero.
 * prev and cur: HOST images of the same rows, cols and format, each with its own pitch (0: packed), with the pointer, pitch
 * and alignment rules of ppf_cloud_from_depth; dp is its format, depth_scale, z_min, z_max (flags is ignored); intr = {fx,
 * fy, ppx, ppy}.  init16: row-major 4 x 4 doubles, all finite, or NULL.  pose16 (16 doubles) is required; level_rows (4 rows,
 * one per level 0..3) and stats may be NULL.  Checked in this order, all PPF_ERR_INVALID before any device work: pose16, mp, dp
 * or intr NULL; prev; cur; the intrinsics; init16; the fields of mp against the ranges stated beside them; the image against
 * `levels`.  Without a device the call is PPF_ERR_HIP.  On any error pose16 is init16 (or the identity), the rows and *stats
 * are zero.  The launch count depends on levels, iters and the image size only (evaluations are enqueued ahead; those behind
 * the end of their level or of the call return at a device-side state word); one blocking wait.  No float atomics: the result
 * does not depend on scheduling. */
ppf_status ppf_depth_motion(const void* prev, size_t prev_pitch_bytes, const void* cur, size_t cur_pitch_bytes, int rows, int cols,
                            const double* intr, const ppf_depth_params* dp, const ppf_depth_motion_params* mp, const double* init16,
                            double* pose16, ppf_depth_motion_level* level_rows, ppf_depth_motion_stats* stats);
/* the same from DEVICE images: enqueued on `stream` (a hipStream_t, NULL: default stream), returns when the pose is complete.
 * pose16, level_rows and stats are host memory as above.  An image pointer the current device cannot read, an image that
 * runs past the end of its allocation, or two images that overlap are PPF_ERR_INVALID before anything is launched. */
ppf_status ppf_depth_motion_device(const void* d_prev, size_t prev_pitch_bytes, const void* d_cur, size_t cur_pitch_bytes, int rows,
                                   int cols, const double* intr, const ppf_depth_params* dp, const ppf_depth_motion_params* mp,
                                   const double* init16, void* stream, double* pose16, ppf_depth_motion_level* level_rows,
                                   ppf_depth_motion_stats* stats);

/* ---- posed depth images fused into a truncated signed distance volume: integrate, raycast, extract ---- */
#define PPF_VOLUME_MAX_DIM 1024
#define PPF_VOLUME_MAX_WEIGHT 65535
#define PPF_VOLUME_MAX_STEPS 4096 /* samples of a raycast walk */
#define PPF_VOLUME_MAX_TILES 16777215 /* 16 x 16 pixel tiles of a raycast image: ceil(rows / 16) * ceil(cols / 16) */
typedef struct ppf_depth_volume_params {
  int32_t dims[3];    /* nx, ny, nz, each 1..1024; default 256 each */
  float voxel;        /* metres, finite, > 0; default 0.004 */
  double origin[3];   /* finite: world coordinates of the centre of voxel (0, 0, 0); default {-0.510, -0.510, 0.302}: a 1.024 m cube on
                         the optical axis that starts 0.3 m out */
  float trunc;        /* metres, finite, >= voxel; default 0.016 */
  int32_t max_weight; /* 1..65535; default 64 */
  int32_t flags;      /* 0 */
  int32_t reserved[4];
} ppf_depth_volume_params;
typedef struct ppf_depth_volume_voxel {
  float d;   /* the truncated signed distance in units of trunc, -1..1: > 0 in front of the surface */
  int32_t w; /* observations, capped at max_weight; 0: unobserved, d = 1.0f */
} ppf_depth_volume_voxel;
typedef struct ppf_depth_volume_desc {
  int32_t dims[3];
  float voxel;
  double origin[3];
  float trunc;
  int32_t max_weight;
  int64_t integrations; /* successful integrations since creation or the last reset */
  uint64_t device_bytes;
  int32_t reserved[4];
} ppf_depth_volume_desc;
typedef struct ppf_depth_volume_integrate_stats {
  int64_t n_updated;    /* voxels the call updated */
  int32_t n_launches;   /* 1 */
  int32_t n_host_syncs; /* 1 */
  float ms_wall;
  int32_t reserved[4];
} ppf_depth_volume_integrate_stats;
typedef struct ppf_depth_volume_raycast_params {
  float z_near, z_far; /* metres along the optical axis, finite, 0 < z_near < z_far; default 0.3, 1.5 */
  float ray_step;      /* the step as a share of trunc, in (0, 1]; default 0.5 */
  int32_t min_weight;  /* >= 1; default 1 */
  int32_t flags;       /* 0 */
  int32_t reserved[4];
} ppf_depth_volume_raycast_params;
typedef struct ppf_depth_volume_raycast_stats {
  int32_t n_hits;
  int32_t n_interpolated; /* the hits whose bracket came from tri */
  int32_t n_launches;     /* 1 */
  int32_t n_host_syncs;   /* 1 */
  float ms_wall;
  int32_t reserved[4];
} ppf_depth_volume_raycast_stats;
typedef struct ppf_depth_volume_extract_params {
  int32_t min_weight; /* >= 1; default 1 */
  int32_t flags;      /* 0 */
  int32_t reserved[4];
} ppf_depth_volume_extract_params;
typedef struct ppf_depth_volume_extract_stats {
  int64_t n_crossings;  /* sign changes between two observed, unsaturated neighbours */
  int64_t n_rows;       /* those with a normal: the cloud's rows */
  int32_t n_launches;   /* 7 */
  int32_t n_host_syncs; /* 2: the read-back that sizes the cloud, and the end */
  float ms_wall;
  int32_t reserved[4];
} ppf_depth_volume_extract_stats;
typedef struct ppf_depth_volume ppf_depth_volume;
/* dims 256 256 256, voxel 0.004, origin -0.510 -0.510 0.302, trunc 0.016, max_weight 64, flags 0 */
void ppf_default_depth_volume_params(ppf_depth_volume_params* p);
/* z_near 0.3, z_far 1.5, ray_step 0.5, min_weight 1, flags 0 */
void ppf_default_depth_volume_raycast_params(ppf_depth_volume_raycast_params* p);
/* min_weight 1, flags 0 */
void ppf_default_depth_volume_extract_params(ppf_depth_volume_extract_params* p);
/* A ppf_depth_volume is nx * ny * nz records {float d; int32_t w} on the device, x fastest: voxel (i, j, k) is record
 * (k * ny + j) * nx + i and its centre lies at origin_a + (double)index_a * (double)voxel.  Creation and reset set every record
 * to d = 1.0f, w = 0: unobserved.  A pose argument is pose16: row-major 4 x 4 doubles T, all finite, world -> camera; R and t
 * are its rotation and translation.  Everything below is fp64 as written, left to right, nothing fused; voxel and trunc enter
 * as (double) of the floats; z(p) and "kept" are ppf_cloud_from_depth's; dp->flags is ignored.
 *
 * INTEGRATE, per voxel (i, j, k):
 *  1. P0 = origin[0] + (double)i * voxel, P1 and P2 likewise with j and k.
 *  2. p_r = ((T[r][0] P0 + T[r][1] P1) + T[r][2] P2) + T[r][3].
 *  3. The voxel is skipped unless p2 > 0; uf = floor((p0 * fx / p2 + ppx) + 0.5) and vf likewise with p1, fy, ppy satisfy, as
 *     doubles, 0 <= uf < cols and 0 <= vf < rows (a NaN satisfies nothing); and the pixel (uf, vf) is kept.  Z = (double)z.
 *  4. sdf = Z - p2; the voxel is skipped when sdf < -trunc.
 *  5. dn = sdf / trunc, and 1.0 when that is larger than 1.0.
 *  6. d <- (float)(((double)d * (double)w + dn) / (double)(w + 1)); w <- min(w + 1, max_weight).
 * A skipped voxel keeps its bytes.  n_updated counts the others.
 *
 * RAYCAST makes an image of the caller's rows, cols and intr, which need not be an input's.  step = (double)ray_step * trunc,
 * K = ceil(((double)z_far - (double)z_near) / step); K > PPF_VOLUME_MAX_STEPS is an argument error.  Per image
 * c_a = -((R[0][a] t0 + R[1][a] t1) + R[2][a] t2).  Per pixel (u, v): dc = (((double)u - ppx) / fx, ((double)v - ppy) / fy, 1),
 * dw_a = (R[0][a] dc0 + R[1][a] dc1) + R[2][a] dc2, point(s)_a = c_a + s * dw_a: s is the camera-frame depth.
 *   near(P): the voxel floor((P_a - origin_a) / voxel + 0.5) per axis; "none" when it is outside the volume (compared as
 *     doubles) or its w < min_weight, else (double)d.
 *   tri(P): g_a = (P_a - origin_a) / voxel, b_a = floor(g_a), f_a = g_a - b_a; "none" unless all eight voxels b + {0,1}^3 are
 *     inside the volume with w >= min_weight; else seven lerps lo + f * (hi - lo): four along x (f_0), then two along y of
 *     those, then one along z.
 * The walk: s_k = z_near + (double)k * step for k = 0 .. K - 1; a sample is front when near gives a value > 0, back when it
 * gives a value <= 0, neither when it gives none.  The walk ends at the first back sample k; the pixel is a hit iff k >= 1
 * and sample k - 1 was front.  For a hit a0 = tri(point(s_{k-1})), a1 = tri(point(s_k)); when both exist and a0 > 0 >= a1 they
 * are (f0, f1) and the hit counts in n_interpolated, else the two near values are.  s* = s_{k-1} + step * f0 / (f0 - f1); the
 * depth written is (float)s*, every other pixel gets 0.0f: a PPF_DEPTH_F32 image for every depth stage.  The optional normals
 * image (packed rows x cols x 3 floats) is, with P* = point(s*): g_a = tri(P* + voxel e_a) - tri(P* - voxel e_a),
 * len = sqrt((g0 g0 + g1 g1) + g2 g2); zeros when any of the six is none or len is 0 (or the pixel is no hit); else
 * n_w = g / len and n_r = (R[r][0] n_w0 + R[r][1] n_w1) + R[r][2] n_w2 cast to float: camera coordinates, nothing flipped.
 *
 * EXTRACT, for every voxel in linear order and for the axes x, y, z in that order: m is the voxel one step along the axis and
 * must be inside the volume; both have w >= min_weight and fabs((double)d) < 1 (saturated free space is no surface); and
 * (d0 > 0) != (d1 > 0): a crossing.  t = (double)d0 / ((double)d0 - (double)d1); the point is the voxel's centre with
 * t * voxel added along the axis.  The gradient at a lattice voxel is (double)d(+e_a) - (double)d(-e_a) per axis and needs its
 * six neighbours inside the volume with w >= min_weight (nothing else is asked of them); g = g(voxel) + t * (g(m) - g(voxel)),
 * len = sqrt((g0 g0 + g1 g1) + g2 g2), the normal g / len.  A crossing gives no row when either gradient is undefined or len
 * is 0.  The cloud's rows are x y z nx ny nz as floats in world coordinates, curvature 0, in (linear voxel index, axis) order;
 * no row gives an empty cloud.
 *
 * Calls on one volume are serialised inside the library; different volumes may be used from different threads.
 *
 * create: out, then vp NULL; dims; voxel; origin; trunc; max_weight; flags -- PPF_ERR_INVALID in this order, before any
 * device work; then PPF_ERR_HIP without a device; a volume that cannot be allocated is PPF_ERR_NOMEM.  *out is NULL on any
 * error. */
ppf_status ppf_depth_volume_create(const ppf_depth_volume_params* vp, ppf_depth_volume** out);
/* A test surface: create's argument checks and a handle that holds the params and no device memory, made without asking for a
 * device.  _info and _release take it; every other entry checks its arguments as on a real volume and then, where a real one
 * would start its device work, is PPF_ERR_HIP without a device and PPF_ERR_INVALID with one. */
ppf_status ppf_debug_depth_volume_shell(const ppf_depth_volume_params* vp, ppf_depth_volume** out);
ppf_status ppf_depth_volume_release(ppf_depth_volume* v);
/* every record back to {1.0f, 0}, integrations to 0 */
ppf_status ppf_depth_volume_reset(ppf_depth_volume* v);
/* the params of creation, the integrations since the last reset and the device memory held */
ppf_status ppf_depth_volume_info(const ppf_depth_volume* v, ppf_depth_volume_desc* info);
/* the nx * ny * nz records to HOST memory in linear order: a plain blocking copy.  n_voxels must be nx * ny * nz. */
ppf_status ppf_depth_volume_read(const ppf_depth_volume* v, ppf_depth_volume_voxel* out, size_t n_voxels);
/* Integrate a HOST image with the pointer, pitch and alignment rules of ppf_cloud_from_depth; intr = {fx, fy, ppx, ppy}.
 * Checked in this order, all PPF_ERR_INVALID before any device work: v NULL; pose16 NULL; dp or intr NULL; the image as
 * ppf_cloud_from_depth checks it (depth NULL, size, format, pitch, alignment, depth_scale, z range); the intrinsics; pose16
 * finite.  Then PPF_ERR_HIP without a device.  One launch and one blocking wait whatever the image holds.  On any error the
 * volume keeps its bytes, its integrations do not advance and *stats is zero. */
ppf_status ppf_depth_volume_integrate(ppf_depth_volume* v, const void* depth, int rows, int cols, size_t row_pitch_bytes,
                                      const double* intr, const ppf_depth_params* dp, const double* pose16,
                                      ppf_depth_volume_integrate_stats* stats /* may be NULL */);
/* the same from a DEVICE image: enqueued on `stream` (a hipStream_t, NULL: default stream), returns when the volume is
 * complete.  After the checks above: an image the current device cannot read, one that runs past the end of its allocation
 * or one that overlaps the volume is PPF_ERR_INVALID before anything is launched. */
ppf_status ppf_depth_volume_integrate_device(ppf_depth_volume* v, const void* d_depth, int rows, int cols, size_t row_pitch_bytes,
                                             const double* intr, const ppf_depth_params* dp, const double* pose16, void* stream,
                                             ppf_depth_volume_integrate_stats* stats /* may be NULL */);
/* Raycast into HOST memory: depth_out packed rows x cols floats, normals_out packed rows x cols x 3 floats or NULL.  Checked in
 * this order, all PPF_ERR_INVALID before any device work: v; depth_out; pose16; rp; intr NULL; rows, cols; the intrinsics;
 * pose16 finite; z_near and z_far; ray_step; min_weight; flags; K; more than PPF_VOLUME_MAX_TILES tiles (a launch holds fewer
 * than 2^32 lanes).  Then PPF_ERR_HIP without a device.  One launch and one
 * blocking wait whatever the volume holds.  On any error the outputs are not touched and *stats is zero. */
ppf_status ppf_depth_volume_raycast(ppf_depth_volume* v, int rows, int cols, const double* intr, const double* pose16,
                                    const ppf_depth_volume_raycast_params* rp, float* depth_out, float* normals_out /* may be NULL */,
                                    ppf_depth_volume_raycast_stats* stats /* may be NULL */);
/* the same into DEVICE buffers, on `stream`.  After the checks above: an output the current device cannot write or that runs
 * past the end of its allocation (the depth output, then the normals), an output that overlaps the volume, or the normals
 * overlapping the depth output, is PPF_ERR_INVALID before anything is launched. */
ppf_status ppf_depth_volume_raycast_device(ppf_depth_volume* v, int rows, int cols, const double* intr, const double* pose16,
                                           const ppf_depth_volume_raycast_params* rp, float* d_depth, float* d_normals /* may be NULL */,
                                           void* stream, ppf_depth_volume_raycast_stats* stats /* may be NULL */);
/* The zero surface as a ppf_cloud, as ppf_cloud_from_depth_normals returns one (release it with ppf_cloud_release): what
 * the cloud stages take, and downloaded what ppf_model_train takes.  Checked in this order: out; v; ep NULL; min_weight; flags (PPF_ERR_INVALID),
 * then PPF_ERR_HIP without a device.  Seven launches and two blocking waits whatever the volume holds.  On any error *out is
 * NULL and *stats is zero. */
ppf_status ppf_depth_volume_extract(ppf_depth_volume* v, const ppf_depth_volume_extract_params* ep, ppf_cloud** out,
                                    ppf_depth_volume_extract_stats* stats /* may be NULL */);
/* The inverse of _read: nx * ny * nz records from HOST memory in linear order replace the volume's, a plain blocking copy
 * under the volume's lock: a saved scan restored, or a chosen state for a test.  Checked on the host in this order, all
 * PPF_ERR_INVALID before any device work: v NULL; in NULL; n_voxels != nx * ny * nz; the first record with w outside
 * 0 .. max_weight or with d not finite or outside [-1, 1] (the message names its linear index).  Then PPF_ERR_HIP without a
 * device.  On any error the volume keeps its bytes; integrations is not changed by a write. */
ppf_status ppf_depth_volume_write(ppf_depth_volume* v, const ppf_depth_volume_voxel* in, size_t n_voxels);

/* ---- the volume's zero surface as a triangle mesh, by marching tetrahedra ------------------------------ */
typedef struct ppf_depth_volume_mesh_params {
  int32_t min_weight; /* >= 1; default 1 */
  int32_t flags;      /* 0 */
  int32_t reserved[4];
} ppf_depth_volume_mesh_params;
typedef struct ppf_depth_volume_mesh_stats {
  int64_t n_cells;      /* active cubes */
  int64_t n_vertices;
  int64_t n_triangles;
  int64_t n_no_normal;  /* vertices whose normal is 0 0 0 */
  int32_t n_launches;   /* 14 */
  int32_t n_host_syncs; /* 2: the read-back that sizes the mesh, and the end */
  float ms_wall;
  int32_t reserved[4];
} ppf_depth_volume_mesh_stats;
typedef struct ppf_volume_mesh ppf_volume_mesh; /* vertices and triangles, resident on the device */
typedef struct ppf_volume_mesh_desc {
  int64_t n_vertices;
  int64_t n_triangles;
  uint64_t device_bytes;
  int32_t reserved[4];
} ppf_volume_mesh_desc;
/* min_weight 1, flags 0 */
void ppf_default_depth_volume_mesh_params(ppf_depth_volume_mesh_params* p);
/* MESH.  Everything is fp64 as written, left to right, nothing fused.  A voxel is valid iff w >= min_weight and
 * fabs((double)d) < 1, and positive iff (double)d > 0.  A cube is (i, j, k) with 0 <= i < nx - 1, 0 <= j < ny - 1,
 * 0 <= k < nz - 1 (a volume with a dimension of 1 has none); its corner c in 0..7 is the voxel
 * (i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1)).  A cube is active iff all eight corners are valid; only active cubes
 * give triangles.
 *   Each cube has six tetrahedra, the monotone paths 0 -> 7 of the axis permutations in lexicographic order; corners
 *   (t0, t1, t2, t3): (0,1,3,7) (0,1,5,7) (0,2,3,7) (0,2,6,7) (0,4,5,7) (0,4,6,7).
 *   In a tetrahedron P is the set of positive corners and N the rest, both in path order.  |P| of 0 or 4 gives nothing.  A lone
 *   corner a (|P| = 1 or |N| = 1) with the others b1, b2, b3 gives one triangle (E(a,b1), E(a,b2), E(a,b3)).  N = {a1, a2} and
 *   P = {b1, b2} give two, in this order: (E(a1,b1), E(a1,b2), E(a2,b2)) and (E(a1,b1), E(a2,b2), E(a2,b1)).
 *   Orientation: with every E at its edge's midpoint in the unit cube and m = mean of the P corners - mean of the N corners,
 *   v1 and v2 are swapped when ((v1 - v0) x (v2 - v0)) . m < 0 (it is never 0: the midpoint surface is the zero set of the
 *   affine function that is +1 on P and -1 on N).  Triangles are counter-clockwise seen from the free-space side.
 *   E(ca, cb), the bits of ca inside those of cb, lies on the edge owned by the voxel at corner ca; the edge's type is
 *   e = (ca ^ cb) - 1: 0 x, 1 y, 2 xy, 3 z, 4 xz, 5 yz, 6 xyz.  The vertex (p, e) exists iff a triangle names it, which is
 *   exactly when the edge's two end voxels differ in `positive` and at least one active cube contains the edge.
 *   With d0 = (double)d(p), d1 = (double)d of the other end and t = d0 / (d0 - d1), the position is the centre of p with
 *   t * voxel added to every axis the direction has a 1 in, and the normal is EXTRACT's: g = g(p) + t * (g(end) - g(p)) from
 *   the lattice gradients (six neighbours inside the volume with w >= min_weight), len = sqrt((g0 g0 + g1 g1) + g2 g2), g / len;
 *   0 0 0 when either gradient is undefined or len is not > 0, counted in n_no_normal.
 * Vertices are rows x y z nx ny nz as floats in world coordinates, in (owner's linear voxel index, type) order; triangles are
 * three int32 vertex indices each, in (cube's corner-0 linear voxel index, tetrahedron, triangle) order.  No atomic decides a
 * place.
 *
 * Checked in this order: out NULL (otherwise *out = NULL); v; mp NULL; min_weight < 1; flags != 0 (PPF_ERR_INVALID), then
 * PPF_ERR_HIP without a device.  More than INT32_MAX vertices or triangles is PPF_ERR_NOMEM, decided by 64-bit counts.
 * Fourteen launches and two blocking waits (the read-back that sizes the mesh, and the end) whatever the volume holds.  On any
 * error *out is NULL and *stats is zero.  An empty result is a valid mesh of 0 vertices and 0 triangles. */
ppf_status ppf_depth_volume_mesh(ppf_depth_volume* v, const ppf_depth_volume_mesh_params* mp, ppf_volume_mesh** out,
                                 ppf_depth_volume_mesh_stats* stats /* may be NULL */);
/* the counts and the device memory held; m or info NULL is PPF_ERR_INVALID */
ppf_status ppf_volume_mesh_info(const ppf_volume_mesh* m, ppf_volume_mesh_desc* info);
/* vertices (n_vertices x 6 floats) and triangles (n_triangles x 3 int32) to HOST memory: plain blocking copies.  Checked in
 * this order, PPF_ERR_INVALID: m NULL; the counts are not the mesh's; vertices NULL with n_vertices > 0; triangles NULL with
 * n_triangles > 0.  An empty mesh accepts NULL pointers. */
ppf_status ppf_volume_mesh_read(const ppf_volume_mesh* m, float* vertices, size_t n_vertices, int32_t* triangles, size_t n_triangles);
ppf_status ppf_volume_mesh_release(ppf_volume_mesh* m);

/* ---- a mesh's connected components: counted, measured, ranked by area, scraps removed ------------------- */
typedef struct ppf_mesh_component_params {
  int32_t min_triangles; /* >= 1; default 1 */
  float min_area;        /* m^2, finite and >= 0; default 0 */
  int32_t rank_lo;       /* >= 0; default 0 */
  int32_t rank_hi;       /* >= rank_lo; default INT32_MAX */
  int32_t flags;         /* 0 */
  int32_t reserved[3];
} ppf_mesh_component_params;
typedef struct ppf_mesh_component_info {
  int32_t n_vertices;
  int32_t n_triangles;         /* degenerate ones included */
  int32_t n_degenerate;
  int32_t n_edges;             /* distinct edges of the non-degenerate triangles */
  int32_t n_boundary_edges;    /* held by one triangle; 0: the component is closed */
  int32_t n_nonmanifold_edges; /* held by more than two */
  int32_t first_vertex;        /* the component's smallest vertex index */
  int32_t kept;                /* 0 | 1 */
  double area;                 /* m^2: area_q * 2^-40 */
  float lo[3], hi[3];          /* the bounds of the vertex positions */
  int32_t reserved[2];
} ppf_mesh_component_info;
typedef struct ppf_mesh_component_stats {
  int64_t n_components;
  int64_t n_kept;
  int64_t n_unreferenced;  /* vertices that no triangle names */
  int64_t n_bad_area;      /* triangles whose area has no integer form */
  int64_t n_vertices_out;  /* of the output mesh, also when out is NULL */
  int64_t n_triangles_out;
  int32_t n_launches;      /* 82, or 80 when out is NULL */
  int32_t n_host_syncs;    /* 2: the read-back that sizes the output, and the end */
  float ms_wall;
  int32_t reserved[5];
} ppf_mesh_component_stats;

/* A ppf_volume_mesh from HOST arrays, so that a loaded PLY can be cleaned and a test can state a mesh: n_vertices rows of
 * vstride floats whose first three are x y z and whose floats normal_offset .. normal_offset + 2 are the normal (-1: no
 * normals, the rows get 0 0 0), and n_triangles x 3 int32 vertex indices.  The mesh's rows are x y z nx ny nz, every float as
 * given.  Checked on the host in this order, all PPF_ERR_INVALID with a message that names the first offender: out NULL
 * (otherwise *out = NULL); a negative count, or one above INT32_MAX; vertices NULL with n_vertices > 0, triangles NULL with
 * n_triangles > 0; vstride < 3, or normal_offset < -1 or normal_offset + 3 > vstride; the first row with a position that is not
 * finite (its index is named); the first triangle with an index outside [0, n_vertices) (the triangle is named).  Then
 * PPF_ERR_HIP without a device.  0 vertices and 0 triangles are a valid empty mesh and accept NULL pointers. */
ppf_status ppf_volume_mesh_upload(const float* vertices, int64_t n_vertices, int32_t vstride, int32_t normal_offset,
                                  const int32_t* triangles, int64_t n_triangles, ppf_volume_mesh** out);
/* A test surface, like ppf_debug_depth_volume_shell: a handle that holds the counts and no device memory, made without asking
 * for a device.  _info and _release take it; ppf_volume_mesh_components checks its arguments as on a real mesh and then is
 * PPF_ERR_HIP without a device and PPF_ERR_INVALID with one. */
ppf_status ppf_debug_volume_mesh_shell(int64_t n_vertices, int64_t n_triangles, ppf_volume_mesh** out);
/* min_triangles 1, min_area 0, rank_lo 0, rank_hi INT32_MAX, flags 0: everything is kept */
void ppf_default_mesh_component_params(ppf_mesh_component_params* p);
/* COMPONENTS.  A triangle is degenerate when two of its three indices are equal.  A vertex is referenced when any triangle
 * names it, degenerate ones included.  The components are the classes of the smallest equivalence on the referenced vertices in
 * which every triangle's three vertices are equivalent; a triangle belongs to its vertices' component; first_vertex is the
 * component's smallest vertex index.  An unreferenced vertex belongs to no component: its label is -1, it counts in
 * n_unreferenced and never reaches the output.
 *   Area.  Per triangle in fp64 exactly as written, nothing fused: a = (double)p1 - (double)p0 and b = (double)p2 - (double)p0
 *   per axis, c = (ay*bz - az*by, az*bx - ax*bz, ax*by - ay*bx), A = 0.5 * sqrt((cx*cx + cy*cy) + cz*cz).  Its integer form is
 *   q = (uint64)floor(A * 2^40); when A is not finite or A * 2^40 >= 2^63, q is 0 and the triangle counts in n_bad_area.  A
 *   component's area_q is the sum of its triangles' q in uint64 (it wraps at 2^24 m^2), and area = (double)area_q * 2^-40.  The
 *   sum is over integers so that it does not depend on the order and needs no float atomic.
 *   Edges.  The edges of a non-degenerate triangle are the unordered pairs {i0,i1} {i1,i2} {i2,i0}; an edge's multiplicity is
 *   the number of non-degenerate triangles that hold it.  n_edges counts the distinct edges, n_boundary_edges those of
 *   multiplicity 1, n_nonmanifold_edges those above 2.  A component is closed iff n_boundary_edges == 0, and its Euler
 *   characteristic is n_vertices - n_edges + n_triangles (without the degenerate ones, where there are any).
 *   lo / hi.  The minima and maxima of the component's vertex positions as floats, -0 below +0.
 *   Rank.  The components ordered by (area_q descending, first_vertex ascending) have the ranks 0 .. C - 1.
 *   Kept.  A component is kept iff rank_lo <= rank < rank_hi, n_triangles >= min_triangles and area >= (double)min_area.
 *   Output.  The kept components' vertex rows in input order, every byte unchanged, normals included; the kept triangles in
 *   input order, each index replaced by the number of kept vertices before it.  No atomic decides a place.  With everything
 *   kept and no unreferenced vertex the output equals the input byte for byte.
 *   labels[v] is the rank of v's component, or -1.  info[r] describes the component of rank r, for r below min(C, cap_info);
 *   the records from C on are left as they are.
 *
 * Checked in this order, PPF_ERR_INVALID: out, when given, gets *out = NULL; m NULL; p NULL; min_triangles < 1; min_area
 * negative or not finite; rank_lo < 0; rank_hi < rank_lo; flags != 0; cap_info < 0; info NULL with cap_info > 0.  Then
 * PPF_ERR_HIP without a device.  out NULL measures only: labels, info and stats are as with an output, the two passes that
 * write it are not launched.  82 launches (80 with out NULL) and two blocking waits (the read-back that sizes the output, and
 * the end) whatever the mesh holds.  The input mesh is never written.  On any error *out is NULL and *stats is zero.  Nothing
 * kept is a valid mesh of 0 vertices and 0 triangles. */
ppf_status ppf_volume_mesh_components(const ppf_volume_mesh* m, const ppf_mesh_component_params* p, ppf_volume_mesh** out /* NULL: measure only */,
                                      int32_t* labels /* HOST, n_vertices; may be NULL */, ppf_mesh_component_info* info /* HOST, cap_info */,
                                      int cap_info, ppf_mesh_component_stats* stats /* may be NULL */);

/* ---- a model cloud sampled from a triangle mesh ------------------------------------------------------
 * The CAD side of "where does the model come from": rows x y z nx ny nz drawn on the surface of a triangle mesh, one per
 * spacing^2 on average, without the faces no camera can see and with the normals turned outward.  Everything below is evaluated
 * in fp64 exactly as written (no contraction), so a row's bytes are a function of the arguments alone.
 *
 * mix(x):  x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13; x *= 0xc2b2ae35; x ^= x >> 16          (uint32, mod 2^32)
 * h(seed, k, c) = mix(mix(mix(seed + 0x9e3779b9) ^ k) ^ c)                        (k the triangle, c a counter, uint32)
 * 1. Triangle k = (i0, i1, i2): v = (double) of the vertices' floats, e1 = v1 - v0, e2 = v2 - v0,
 *    c = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), L = sqrt((c0 c0 + c1 c1) + c2 c2).  The triangle is
 *    degenerate iff !(L > 0) or L is not finite (a non-finite vertex makes it so): it is counted in n_degenerate, gives no
 *    rows and draws nothing.  area = the sum of 0.5 L in any order (reported only).
 * 2. q = (0.5 L) / ((double)spacing * (double)spacing), f = floor(q),
 *    n_k = f + ((h(seed, k, 0) >> 8) < (uint32)floor((q - f) * 16777216.0) ? 1 : 0).  q >= max_rows for one triangle, or
 *    the sum of the n_k above max_rows, is PPF_ERR_CAPACITY before any row is made.
 * 3. Row j of triangle k: u = ((double)(h(seed, k, 2j + 1) >> 8) + 0.5) / 16777216.0, v likewise from 2j + 2 (counters
 *    mod 2^32); if u + v > 1.0 then u = 1.0 - u and v = 1.0 - v.  p = (float)((v0 + u e1) + v e2) per component.
 *    PPF_MESH_NORMALS_FACE: n = (float)(c / L).  PPF_MESH_NORMALS_VERTEX: with n0, n1, n2 the (double) vertex normals and
 *    w = (1.0 - u) - v, m = (w n0 + u n1) + v n2 per component and l = sqrt((m0 m0 + m1 m1) + m2 m2): n = (float)(m / l)
 *    when l > 0 and l is finite, the face normal otherwise.
 * 4. Views (visibility only): the 26 directions d are the non-zero vectors of {-1, 0, 1}^3 in lexicographic order with x
 *    slowest, each times 1.0 / sqrt(1.0 | 2.0 | 3.0) by its count of non-zero components.  e = the coordinate axis of the
 *    smallest |d| component (the first on ties), t = d x e, a = t / sqrt((t0 t0 + t1 t1) + t2 t2), b = d x a (cross
 *    products as in 1).  lo, hi = the minima and maxima of the floats of the vertices of non-degenerate triangles (-0 below
 *    +0), ctr = 0.5 (lo + hi), g = hi - lo, r = 0.5 sqrt((g0 g0 + g1 g1) + g2 g2), px = 2.0 r / (double)(R - 2), R = map_size.
 *    A point p maps to X = dot(p - ctr, a) / px + 0.5 R, Y the same with b, D = dot(p - ctr, d) + r; dot(s, t) =
 *    (s0 t0 + s1 t1) + s2 t2.
 * 5. Depth maps: R x R uint32 per view, empty = 0xffffffff.  Every non-degenerate triangle is drawn in every view from the
 *    X, Y and (float)D of its three vertices by the rule of ppf_depth_register's triangles: x0 = ceil(min X), x1 = floor(max X),
 *    y likewise, clamped to 0 .. R - 1, nothing when empty; area2 = (bx - ax)(cy - ay) - (by - ay)(cx - ax), nothing when it
 *    is 0; a pixel (i, j) (X = i, Y = j) is covered iff w0 = (cx - bx)(j - by) - (cy - by)(i - bx), w1 = (ax - cx)(j - cy) -
 *    (ay - cy)(i - cx), w2 = (bx - ax)(j - ay) - (by - ay)(i - ax) are all >= 0 or all <= 0; its value is
 *    z = (float)(((w0 Da + w1 Db) + w2 Dc) / area2), stored as the unsigned minimum of the bit pattern of (z > 0 ? z : +0).
 *    There is no pixel cap.
 * 6. A row is tested with the float p and n it outputs.  Per view: fi = floor(X + 0.5), fj = floor(Y + 0.5); the row is
 *    seen iff (fi, fj) is not a pixel of the map, the pixel is empty, or (double)(float)D <= (double)z + tol, tol =
 *    depth_tol > 0 ? (double)depth_tol : 2.0 px.  seen counts those views, front those of them with dot(n, d) < 0, back
 *    those with > 0.  The row is kept iff seen >= max(1, min_views).  With orient, a kept row with back > front has its
 *    three normal components negated and is counted in n_flipped.
 * 7. Kept rows leave in (k, j) order; curvature is 0.  n_sampled = sum n_k, n_hidden = n_sampled - n_rows.
 *
 * Checked in this order, all PPF_ERR_INVALID before any device work: out NULL (then *out = NULL); p NULL; vertices or
 * triangles NULL; n_vertices < 1 or n_triangles < 1; vstride < 3; normal_offset other than -1 or 3 .. vstride - 3; spacing
 * not finite or <= 0; normals not 0 or 1; PPF_MESH_NORMALS_VERTEX without a normal offset; visibility not 0 or 1; orient
 * not 0 or 1; orient without visibility; map_size not 0 or 16 .. 1024; min_views outside 0 .. 26; depth_tol not finite or
 * < 0; max_rows < 0; reserved != 0; with visibility, 26 n_triangles >= 2^32; the first triangle with an index outside
 * [0, n_vertices).  Then, for a mesh of at most PPF_MESH_HOST_COUNT triangles, the rows are counted on the host and more
 * than max_rows is PPF_ERR_CAPACITY; then PPF_ERR_HIP without a device; larger meshes are counted on the device
 * (PPF_ERR_CAPACITY after the first wait).  Host arrays in, a device-resident cloud out (release it with ppf_cloud_release),
 * which holds the memory of n_sampled rows.  On the null stream; two threads may call at once.  8 launches without
 * visibility, 17 with it, and two blocking waits whatever the mesh holds.  On any error *out is NULL and *stats is zero. */
#define PPF_MESH_NORMALS_FACE 0
#define PPF_MESH_NORMALS_VERTEX 1
#define PPF_MESH_VIEWS 26
#define PPF_MESH_HOST_COUNT 1024
typedef struct ppf_mesh_sample_params {
  float spacing;      /* metres, > 0: on average one row per spacing^2 of surface; default 0.004 */
  uint32_t seed;      /* default 0 */
  int32_t normals;    /* PPF_MESH_NORMALS_FACE | PPF_MESH_NORMALS_VERTEX (needs normal_offset >= 0); default FACE */
  int32_t visibility; /* 0: every sampled row; 1: only rows some view can see; default 1 */
  int32_t map_size;   /* R, side of a view's depth map; 0 = 256; 16..1024 */
  int32_t min_views;  /* 0 = 1; 1..26 */
  float depth_tol;    /* metres; 0 = two map pixels */
  int32_t orient;     /* 1: a row seen more often from behind has its normal negated (needs visibility); default 1 */
  int32_t max_rows;   /* 0 = 1 << 24; more sampled rows than this is PPF_ERR_CAPACITY before any row is made */
  int32_t reserved[4];
} ppf_mesh_sample_params;
typedef struct ppf_mesh_sample_stats {
  int64_t n_triangles;
  int64_t n_degenerate;
  int64_t n_sampled;
  int64_t n_hidden;
  int64_t n_flipped;
  int64_t n_rows;
  int64_t n_large;      /* triangle-view pairs drawn by the large path: a non-empty clamped box of more than 16 pixels a
                           side and area2 != 0 */
  int32_t n_launches;
  int32_t n_host_syncs;
  double area;          /* the mesh's surface, exempt from byte parity: its summation order is free */
  int32_t reserved[4];
} ppf_mesh_sample_stats;
void ppf_default_mesh_sample_params(ppf_mesh_sample_params* p);
ppf_status ppf_cloud_from_mesh(const float* vertices, int n_vertices, int vstride, int normal_offset /* -1: none */,
                               const int32_t* triangles, int n_triangles, const ppf_mesh_sample_params* p, ppf_cloud** out,
                               ppf_mesh_sample_stats* stats /* may be NULL */);

/* ---- a depth image's surfaces labelled in image space: proposals without leaving the image ----------- */
#define PPF_SEGMENT_EIGHT 1      /* flags: 8-connectivity instead of 4 */
#define PPF_SEGMENT_UNORIENTED 2 /* flags: normals agree on |dot|, as PPF_REGION_UNORIENTED */
typedef struct ppf_segment_params {
  float depth_abs;           /* finite, >= 0, metres; default 0.005 */
  float depth_quad;          /* finite, >= 0, 1/metres; default 0 */
  float normal_cos;          /* finite, -1..1; default 0.9659258f; ignored without normals */
  float curvature_threshold; /* >= 0, +inf allowed, not NaN; default 0.03; ignored without normals */
  int32_t min_size;          /* >= 1 pixels; default 100 */
  int32_t max_size;          /* 0: no bound */
  int32_t max_segments;      /* 1..PPF_CLUSTER_MAX_CLUSTERS; default 64 */
  int32_t flags;             /* 0 | PPF_SEGMENT_EIGHT | PPF_SEGMENT_UNORIENTED */
  int32_t reserved[4];
} ppf_segment_params;
typedef struct ppf_segment_info {
  int32_t n_pixels, n_border; /* all its pixels; the attached border pixels among them */
  int32_t first_pixel;        /* v * cols + u of its smallest SMOOTH pixel */
  int32_t box_xywh[4];        /* {umin, vmin, umax - umin, vmax - vmin} over all its pixels: ppf_cluster_info's convention */
  float z_lo, z_hi;           /* the float minimum and maximum of its pixels' z */
  int32_t reserved[3];
} ppf_segment_info;
typedef struct ppf_segment_stats {
  int32_t n_kept, n_eligible, n_smooth, n_attached; /* pixels: kept, eligible, smooth, border pixels that joined a component */
  int32_t n_launches;   /* kernel launches of the call */
  int32_t n_host_syncs; /* blocking waits of the call: 1 */
  float ms_wall;
  int32_t reserved[4];
} ppf_segment_stats;
/* depth_abs 0.005, depth_quad 0, normal_cos 0.9659258, curvature_threshold 0.03, min_size 100, max_size 0, max_segments 64,
 * flags 0 */
void ppf_default_segment_params(ppf_segment_params* p);
/* Connected components of the depth image's own pixel grid, as a closed specification.  Every operation is fp64 as written,
 * nothing fused; z(p) and "kept" are ppf_cloud_from_depth's, Z = (double)z, a pixel's index is v * cols + u; dp->flags is
 * ignored.  Adjacent means the 4 neighbours (+-1 in u or in v), or all 8 with PPF_SEGMENT_EIGHT.
 *   normals == NULL: every kept pixel is eligible and smooth, and agree(p, q) is always true.
 *   normals != NULL: the cloud must be what ppf_cloud_from_depth_normals gives for this image and this dp without
 *     PPF_DEPTH_NORMALS_DROP: row k belongs to the k-th kept pixel in row-major order; only nx ny nz and the curvature are
 *     read.  A pixel is eligible iff it is kept and nx, ny, nz are finite, smooth iff eligible and curvature <=
 *     curvature_threshold (a float comparison: a NaN curvature is not smooth), a border pixel iff eligible and not smooth.
 *     agree(p, q) iff dot >= (double)normal_cos with dot = ((double)pnx*(double)qnx + (double)pny*(double)qny) +
 *     (double)pnz*(double)qnz (fabs(dot) with PPF_SEGMENT_UNORIENTED): ppf_prep_regions' rule.
 *   step(p, q) iff fabs(Zq - Zp) <= (double)depth_abs + (double)depth_quad * (Zp * Zq); it is symmetric.
 * Two adjacent smooth pixels are linked iff step and agree; a component is a connected component of the links.  A border pixel
 * joins the component of the adjacent smooth pixel with the smallest fabs(Zq - Zb) (ties: the smaller pixel index) among those
 * it steps to and agrees with, or no segment; border pixels link nothing.  n_pixels counts a component's smooth and attached
 * border pixels.  A component is valid iff min_size <= n_pixels and (max_size == 0 or n_pixels <= max_size); the valid
 * components ranked by n_pixels descending, then first_pixel ascending, the first min(valid, max_segments) are the segments.
 * labels: packed rows x cols int32, the rank of the pixel's segment or -1.  info: [max_segments], zero past the count.
 * counts: [3] = {segments output, valid components, all components}.  Everything ppf_depth_filter says about depth, the pitch,
 * dp and their errors holds; sp NULL, a field outside the range stated beside it, an unknown flag or labels / info / counts
 * NULL are PPF_ERR_INVALID before any device work too; a normals cloud whose row count is not n_kept is PPF_ERR_INVALID,
 * found at the call's one wait; without a device the call is PPF_ERR_HIP.  The launch count depends on nothing but
 * normals != NULL; one blocking wait (n_host_syncs 1).  On every error info, counts and
 * *stats are zero and labels is not touched.  stats may be NULL. */
ppf_status ppf_depth_segments(const void* depth, int rows, int cols, size_t row_pitch_bytes, const ppf_depth_params* dp,
                              const ppf_cloud* normals /* may be NULL */, const ppf_segment_params* sp, int32_t* labels,
                              ppf_segment_info* info, int32_t* counts, ppf_segment_stats* stats /* may be NULL */);
/* the same between DEVICE buffers, as ppf_depth_filter_device: enqueued on `stream` (a hipStream_t, NULL: default stream),
 * returns when the label image is complete; info, counts and stats stay HOST memory.  A pointer the current device cannot
 * read, a buffer that runs past the end of its allocation, or d_labels overlapping the depth image is PPF_ERR_INVALID before
 * anything is launched; after any other error the content of d_labels is unspecified. */
ppf_status ppf_depth_segments_device(const void* d_depth, int rows, int cols, size_t row_pitch_bytes, const ppf_depth_params* dp,
                                     const ppf_cloud* normals /* may be NULL */, const ppf_segment_params* sp, int32_t* d_labels,
                                     void* stream, ppf_segment_info* info, int32_t* counts, ppf_segment_stats* stats /* may be NULL */);

/* ---- a depth image's occluding and boundary edges: the edge cloud of the depth route ------------------ */
#define PPF_EDGE_OCCLUDING 1  /* p is the near side of a depth step */
#define PPF_EDGE_OCCLUDED  2  /* p is the far side */
#define PPF_EDGE_BOUNDARY  4  /* p borders unmeasured pixels with nothing kept behind them */
#define PPF_EDGE_CURVATURE 8  /* with normals: curvature > curvature_threshold (ppf_prep_edges' rule) */
#define PPF_DEPTH_EDGE_MAX_GAP 8
typedef struct ppf_depth_edge_params {
  float depth_abs;           /* finite, >= 0, metres; default 0.02 */
  float depth_quad;          /* finite, >= 0, 1/metres; default 0 */
  int32_t max_gap;           /* 0..8 not-kept pixels a direction may cross; default 2 */
  float curvature_threshold; /* >= 0, +inf allowed, not NaN; default 0.03; ignored without normals */
  int32_t select;            /* non-zero subset of the four bits: which pixels go to the cloud;
                                default OCCLUDING|BOUNDARY|CURVATURE */
  int32_t flags;             /* none defined: 0 */
  int32_t reserved[4];
} ppf_depth_edge_params;
typedef struct ppf_depth_edge_stats {
  int32_t n_kept, n_occluding, n_occluded, n_boundary, n_curvature; /* pixels carrying each bit */
  int32_t n_edge;       /* mask != 0 */
  int32_t n_selected;   /* mask & select != 0 */
  int32_t n_no_normal;  /* selected, normals given, normal not finite: left out of the cloud */
  int32_t n_rows;       /* rows of *out_cloud; 0 when out_cloud is NULL */
  int32_t n_launches, n_host_syncs;
  float ms_wall;
  int32_t reserved[4];
} ppf_depth_edge_stats;
/* depth_abs 0.02, depth_quad 0, max_gap 2, curvature_threshold 0.03, select OCCLUDING | BOUNDARY | CURVATURE, flags 0 */
void ppf_default_depth_edge_params(ppf_depth_edge_params* p);
/* Where the image says a surface ends, as a closed specification.  Every operation is fp64 as written, nothing fused; z(p) and
 * "kept" are ppf_cloud_from_depth's, Z = (double)z.
 *   jump(p, q) iff fabs(Zq - Zp) > (double)depth_abs + (double)depth_quad * (Zp * Zq): the negation of ppf_depth_segments'
 *   step(p, q), so with equal depth_abs / depth_quad two adjacent kept pixels are an edge pair here iff the segments stage
 *   refuses to link them without normals.
 *   The walk.  For a kept p the 8 directions d = (dv, du) are visited in the order (-1,-1) (-1,0) (-1,1) (0,-1) (0,1) (1,-1)
 *   (1,0) (1,1), with q_j = p + j d.  When q_1 is outside the image the direction gives nothing: the image border is no edge,
 *   as in the filter.  Otherwise j runs 1 .. max_gap + 1 and stops at the first kept q_j: when jump(p, q_j) the direction
 *   gives PPF_EDGE_OCCLUDING if Zq > Zp and PPF_EDGE_OCCLUDED if Zq < Zp, and nothing when it does not jump (a hole inside
 *   one surface is no edge).  When the walk leaves the image at some j >= 2, or ends without a kept pixel, the direction
 *   gives PPF_EDGE_BOUNDARY.  The pixel's mask is the OR over the 8 directions; with max_gap 0 every kept pixel beside a
 *   not-kept pixel inside the image is BOUNDARY.
 *   normals != NULL: the cloud must be what ppf_cloud_from_depth_normals gives for this image and this dp without
 *   PPF_DEPTH_NORMALS_DROP: row k belongs to the k-th kept pixel in row-major order.  PPF_EDGE_CURVATURE is set iff the row's
 *   curvature > curvature_threshold (a float comparison: NaN does not set it).
 * edges: packed rows x cols uint8, 0 at pixels that are not kept.  *out_cloud: the pixels with mask & select != 0 in row-major
 * pixel order (np.nonzero(mask & select) names them); release it with ppf_cloud_release.  With normals a row is the normals
 * cloud's row of that pixel byte for byte -- x y z, the normal, the curvature -- intr is not read and may be NULL, and a
 * selected pixel whose nx, ny, nz are not all finite is left out: it stays in the mask and counts in n_no_normal.  Without
 * normals a row is ppf_cloud_from_depth's row of that pixel, x y z 0 0 0 with curvature 0: dp->flags of 0 | PPF_DEPTH_FP64 is
 * honoured and intr is required.  An empty selection gives an empty cloud.
 *   Checked in this order, all PPF_ERR_INVALID before any device work: out_cloud, when given, gets *out_cloud = NULL; edges
 *   and out_cloud both NULL; ep NULL; intr NULL where it is required; then ppf_cloud_from_depth's checks of depth, the size,
 *   dp, the format, dp->flags (an unknown flag), the pitch, the alignment and depth_scale, of intr where it is required, and
 *   of the z range; then depth_abs, depth_quad, max_gap, curvature_threshold, select (zero, or bits beyond the four), flags.
 *   Without a device the call is PPF_ERR_HIP.  A normals cloud whose row count is not n_kept is PPF_ERR_INVALID, found at
 *   the call's first wait.  On any error *out_cloud is NULL, *stats is zero and edges is untouched.
 * A mask-only call without normals is one launch and one blocking wait.  Normals add the scan of the kept ranks and one pass
 * (7 launches); a cloud adds the scan of the selected ranks, the wait that sizes the cloud and the pass that writes it
 * (7 launches and 2 waits without normals, 13 and 2 with them).  The counts depend on nothing but normals != NULL and
 * out_cloud != NULL.  No atomic decides a place.  Two threads may call at once. */
ppf_status ppf_depth_edges(const void* depth, int rows, int cols, size_t row_pitch_bytes, const double* intr /* may be NULL, see above */,
                           const ppf_depth_params* dp, const ppf_cloud* normals /* may be NULL */, const ppf_depth_edge_params* ep,
                           uint8_t* edges /* may be NULL */, ppf_cloud** out_cloud /* may be NULL */, ppf_depth_edge_stats* stats /* may be NULL */);
/* the same between DEVICE buffers, as ppf_depth_filter_device: enqueued on `stream` (a hipStream_t, NULL: default stream),
 * returns when the mask and the cloud are complete; stats stays HOST memory.  A pointer the current device cannot read, a
 * buffer that runs past the end of its allocation, or d_edges overlapping the depth image is PPF_ERR_INVALID before anything
 * is launched; after any other error the content of d_edges is unspecified. */
ppf_status ppf_depth_edges_device(const void* d_depth, int rows, int cols, size_t row_pitch_bytes, const double* intr /* may be NULL */,
                                  const ppf_depth_params* dp, const ppf_cloud* normals /* may be NULL */, const ppf_depth_edge_params* ep,
                                  uint8_t* d_edges /* may be NULL */, void* stream, ppf_cloud** out_cloud /* may be NULL */,
                                  ppf_depth_edge_stats* stats /* may be NULL */);

/* ---- which trained models a proposal can be a view of: labels for detections nobody named ------------ */
#define PPF_RECOGNIZE_MAX_MODELS 64
#define PPF_RECOGNIZE_MAX_CLOUDS 256
#define PPF_RECOGNIZE_MAX_ROWS 2048
#define PPF_RECOGNIZE_MAX_TOP 16
typedef struct ppf_recognizer ppf_recognizer; /* opaque, immutable, reference counted; retains its models */
typedef struct ppf_recognizer_info {
  int32_t n_rows;    /* the model's sampled rows (ppf_model_info.n_ref) */
  int32_t n_bins[4]; /* n_a, n_a, n_a, n_d: the bins of the key set's four dimensions */
  int32_t in_lds;    /* 1: the scoring kernel stages the set in LDS; 0: it reads it from global memory */
  uint64_t n_keys;   /* the size of the key set */
  uint64_t bytes;    /* what the set takes on the device */
  int32_t reserved[4];
} ppf_recognizer_info;
typedef struct ppf_recognize_params {
  int32_t max_rows;     /* 2..2048; default 512 */
  int32_t top;          /* 1..16; default 2 */
  double min_score;     /* finite, >= 0; default 0 */
  double min_precision; /* finite, >= 0; default 0 */
  int32_t flags;        /* none defined: 0 */
  int32_t reserved[4];
} ppf_recognize_params;
typedef struct ppf_recognize_score {
  int32_t model; /* index into the recogniser's models */
  int32_t reserved;
  uint64_t n_known, n_keys_hit;
  double precision, recall, score;
} ppf_recognize_score;
typedef struct ppf_recognize_stats {
  int32_t n_clouds, n_models;
  int32_t n_launches;   /* kernel launches of the call */
  int32_t n_host_syncs; /* blocking waits of the call: 1 */
  float ms_wall;
  int32_t reserved[4];
} ppf_recognize_stats;
/* Builds every model's key set on the device, once.  models: n_models (1..64) trained models of feature PPF_FEATURE_PPF, under
 * either key_equality, all on the current device; the same model may appear more than once.  A NULL pointer, a count outside
 * its range, a model with fewer than two sampled rows or a PPF_FEATURE_DARBOUX model is PPF_ERR_INVALID before any device work;
 * on every error *out is NULL.  The recogniser retains its models until its last reference is dropped. */
ppf_status ppf_recognizer_create(const ppf_model* const* models, int n_models, ppf_recognizer** out);
ppf_status ppf_recognizer_retain(ppf_recognizer* rec);
ppf_status ppf_recognizer_release(ppf_recognizer* rec); /* NULL is PPF_OK */
ppf_status ppf_recognizer_model_info(const ppf_recognizer* rec, int i, ppf_recognizer_info* info);
/* the key set of model i as tuples, keys4[4q .. 4q + 3], in lexicographic order of the four int32 (INT32_MIN, the bin of a NaN
 * angle, first); *n = its size.  cap (tuples) too small, or keys4 NULL: PPF_ERR_CAPACITY with *n set.  Host only. */
ppf_status ppf_recognizer_keys(const ppf_recognizer* rec, int i, int32_t* keys4, int cap, int* n);
/* max_rows 512, top 2, min_score 0, min_precision 0, flags 0 */
void ppf_default_recognize_params(ppf_recognize_params* p);
/* Scores every proposal cloud against every model of the recogniser and shortlists, per proposal, the models it can be a view
 * of, as a closed specification.  All arithmetic is fp64 as written, nothing fused, with ppf_pair_feature (the table build's
 * pair feature: three deterministic acos of include/ppf_detmath.h and the distance) and ppf_d2i.
 *   Key of an ordered pair of rows i != j (by index: coincident points are pairs like any other) under a model's angle_step and
 *     distance_step (ppf_model_info): with f = {0, 0, 0, 0} and ppf_pair_feature(p_i, n_i, p_j, n_j, f), the tuple
 *     (ppf_d2i(f[0] / angle_step), ppf_d2i(f[1] / angle_step), ppf_d2i(f[2] / angle_step), ppf_d2i(f[3] / distance_step)).
 *     Coordinates and normals are the float rows converted to double, read as they are, with no re-normalisation.  A NaN angle
 *     gives the bin INT32_MIN, a value like any other.  Tuples are compared, not hashes.
 *   Key set of a model: the keys of all ordered pairs of the rows ppf_model_get_sampled returns; n_keys is its size.
 *   Rows of a proposal of n rows: s = ceil(n / max_rows); the candidates are rows 0, s, 2s, ...; the used rows are the
 *     candidates whose six values are all finite, n_used their count, n_pairs = n_used * (n_used - 1).
 *   Per (proposal, model): n_known = the ordered pairs of used rows whose key is in the model's key set; n_keys_hit = the
 *     distinct keys among those pairs; precision = (double)n_known / (double)n_pairs, recall = (double)n_keys_hit /
 *     (double)n_keys, score = precision * recall; all three 0 when n_pairs == 0.  They are computed on the host.
 *   Ranking: the models with score >= min_score and precision >= min_precision, by score descending, then model index
 *     ascending; the first min(top, count) are the proposal's candidates.  A proposal nothing passes has none: clutter.
 * clouds: n_clouds (0..256) pointers; a NULL cloud or one without rows has n_used 0 and no candidates.  n_used: [n_clouds] or
 * NULL.  counts: [n_clouds][n_models][2] = {n_known, n_keys_hit} or NULL.  ranked: [n_clouds][top], zero past a proposal's
 * n_ranked; n_ranked: [n_clouds].  Argument errors (NULL where it is not allowed, a field outside the range stated beside it,
 * an unknown flag, a count outside its range) are PPF_ERR_INVALID before any device work; without a device the call is
 * PPF_ERR_HIP.  On every error n_ranked, ranked, counts, n_used and *stats are zero.  One upload before any device work and one
 * blocking wait (n_host_syncs 1); two launches, whatever n_clouds and the row counts are.  All proposals and models of a call go
 * through one work list built on the host from the row counts.  Each proposal's result is what a call with that cloud alone
 * gives, and it does not depend on scheduling.  stats may be NULL. */
ppf_status ppf_recognize_frame(const ppf_recognizer* rec, const ppf_cloud* const* clouds, int n_clouds, const ppf_recognize_params* p,
                               int32_t* n_used /* may be NULL */, uint64_t* counts /* may be NULL */, ppf_recognize_score* ranked,
                               int32_t* n_ranked, ppf_recognize_stats* stats /* may be NULL */);

/* ---- every detection of a frame in one segmented device pass ------------------------------------------------ */
typedef struct ppf_frame_params {
  double leaf;                /* Subsampling(leafsize), cubic voxel leaf */
  int32_t mean_k;             /* OutlierProcessing(meanK, .) */
  double stddev_mul;          /* OutlierProcessing(., Thresh) */
  int32_t normal_k;           /* NormalEstimation(k) */
  float curvature_threshold;  /* EdgeExtraction(thr) */
  int32_t flags;              /* 0; reserved for later knobs */
  int32_t reserved[4];
} ppf_frame_params;

typedef struct ppf_frame_stats {
  int32_t n_boxes;
  int32_t n_launches;   /* kernel launches enqueued by the call */
  int32_t n_host_syncs; /* blocking D2H copies + stream/device synchronisations made by the call */
  float ms_wall;
  int32_t reserved[4];
} ppf_frame_stats;

/* leaf 0.003, mean_k 50, stddev_mul 1.0, normal_k 30, curvature_threshold 0.03 */
void ppf_default_frame_params(ppf_frame_params* p);
/* SceneCropping -> Subsampling -> OutlierProcessing -> NormalEstimation -> EdgeExtraction -> PointCloudXYZNormalToMat
 * for n_boxes (0..256) boxes {x, y, width, height} of one frame at once.  objects[i] / edges[i] (edges may be NULL)
 * receive box i's to-Mat object and edge clouds (curvature kept), bit-identical to running the single-box ppf_prep_*
 * chain on box i; overlapping boxes share scene rows as they would there.  stage_rows (may be NULL): [n_boxes][4] =
 * rows after crop, voxel grid, outlier removal, edge extraction.  stats may be NULL.  The launch count and the (at
 * most three) host synchronisations do not depend on n_boxes.  The outputs may share one device block: release them
 * in any order.  On error no output is allocated and every output pointer is NULL. */
ppf_status ppf_prep_frame(const ppf_cloud* scene, const int* boxes_xywh, int n_boxes, const float* depth, int depth_rows,
                          int depth_cols, const double* intr, const ppf_frame_params* params, ppf_cloud** objects,
                          ppf_cloud** edges, int32_t* stage_rows, ppf_frame_stats* stats);

/* ---- match + ICP for every detection of a frame, the ICP of all detections in one launch sequence ------------- */
typedef struct ppf_frame_detection {
  const ppf_model* model;       /* NULL: detection skipped (n_out[i] = 0) */
  const ppf_cloud* model_cloud; /* ICP source: the model's full cloud (what registerModelToScene gets as models[id]) */
  const ppf_cloud* scene;       /* the detection's object cloud, e.g. ppf_prep_frame objects[i] */
  const ppf_cloud* edge;        /* NULL: match; else match_S2B against this edge cloud */
} ppf_frame_detection;

typedef struct ppf_match_frame_stats {
  int32_t n_dets, n_matched, n_icp_jobs;
  int32_t n_icp_launches;   /* kernel launches of the ICP phase */
  int32_t n_icp_passes;     /* (neighbour search, tail) pairs launched, summed over levels */
  int32_t n_host_syncs;     /* blocking read-backs + stream/device synchronisations of the whole call */
  float ms_wall, ms_match, ms_icp;
  int32_t reserved[4];
} ppf_match_frame_stats;

/* For every detection: match (or match_S2B) with `mp`, then ICP with `ip` of its first min(top, matches) clustered
 * poses. out is [n_dets][top] poses in match rank order, refined (the reference returns row 0). n_out[i] is the
 * count per detection. icp_iterations is [n_dets][top] and may be NULL; so may stats.
 * Each detection's rows are bit-identical to ppf_match_clouds followed by ppf_icp_refine_clouds on the same clouds.
 * Limits: n_dets 0..256, top 1..16.  A detection whose scene (or given edge cloud) has no rows is skipped like one
 * without a model.  Argument errors are reported before any device work; on any error every n_out[i] is 0.
 * The ICP poses of all detections advance through one launch sequence of up to 256 poses (its launch count does not
 * depend on how many detections share it); a call with more poses runs sequences of 256 one after another.  The match
 * phase reads back per detection. */
ppf_status ppf_match_frame(const ppf_frame_detection* dets, int n_dets, const ppf_match_params* mp,
                           const ppf_icp_params* ip, int top, ppf_pose* out, int* n_out, int32_t* icp_iterations,
                           ppf_match_frame_stats* stats);

/* ---- pose verification: score and re-rank the refined poses of every detection of a frame --------------------- */
#define PPF_VERIFY_ALL_ROWS 1 /* every finite model row counts, not only those facing the camera (scenes that are not one view) */
#define PPF_VERIFY_NORMALS 2  /* a supporting scene row must also agree in normal: cos >= normal_cos */

typedef struct ppf_verify_params {
  float inlier_dist;  /* metres, finite, > 0 */
  float normal_cos;   /* used with PPF_VERIFY_NORMALS, in [-1, 1] */
  float depth_tol;    /* metres, finite, > 0 (checked only with a depth image) */
  int32_t model_step; /* rows 0, s, 2s, ... of the model cloud are scored, >= 1 */
  int32_t flags;      /* 0 | PPF_VERIFY_ALL_ROWS | PPF_VERIFY_NORMALS */
  int32_t reserved[4];
} ppf_verify_params;

typedef struct ppf_pose_score {
  int32_t n_rows;       /* model rows scored: ceil(n_model / model_step) */
  int32_t n_considered; /* finite rows that face the camera (all finite rows with PPF_VERIFY_ALL_ROWS) */
  int32_t n_inliers;    /* considered rows with a supporting scene row */
  int32_t n_visible;    /* considered rows that land on a valid depth pixel (0 without a depth image) */
  int32_t n_supported, n_occluded, n_violations; /* a partition of n_visible */
  float inlier_rmse;    /* metres */
  float fitness;        /* n_inliers / n_considered */
  float support;        /* n_supported / (n_visible - n_occluded); 0 without a depth image */
  float score;          /* support with a depth image, else fitness: what `best` ranks by */
  int32_t reserved[3];
} ppf_pose_score;

typedef struct ppf_verify_stats {
  int32_t n_dets, n_jobs; /* detections given, poses scored */
  int32_t n_launches;     /* kernel launches of the call */
  int32_t n_host_syncs;   /* blocking read-backs + synchronisations of the call (host-to-device uploads not counted) */
  float ms_wall;
  int32_t reserved[4];
} ppf_verify_stats;

/* inlier_dist 0.005, normal_cos 0.5, depth_tol 0.01, model_step 1, flags 0 */
void ppf_default_verify_params(ppf_verify_params* p);
/* Scores pose k < n_poses[i] of detection i: the rows 0, s, 2s, ... of dets[i].model_cloud are moved by poses[i * top + k]
 * (ppf_transform_pc_pose's arithmetic) and tested against dets[i].scene (cloud support: a scene row within inlier_dist)
 * and, when `depth` is given, against the depth image (supported / occluded / free-space violation within depth_tol);
 * DESIGN.md §14 states every test bit for bit.  dets, poses and n_poses are what ppf_match_frame took and returned
 * (model and edge are ignored); poses and scores are [n_dets][top], score rows with k >= n_poses[i] are zero.
 * best[i] is the k with the largest score, the lowest k among equal ones, -1 when n_poses[i] == 0.
 * depth: optional HOST image, float32 metres, packed depth_rows x depth_cols, intr = {fx, fy, ppx, ppy} as ppf_prep_frame
 * takes them; NULL: no depth test (intr may then be NULL).  A pose's score row does not depend on the other poses and
 * detections of the call.  Limits: n_dets 0..256, top 1..16, n_poses[i] 0..top.  Argument errors are PPF_ERR_INVALID
 * before any device work; on any error every score row is zero and every best[i] is -1.  stats may be NULL.  The launch
 * count does not depend on n_dets; the one read-back is the scores. */
ppf_status ppf_verify_frame(const ppf_frame_detection* dets, int n_dets, const ppf_pose* poses, const int* n_poses, int top,
                            const float* depth, int depth_rows, int depth_cols, const double* intr,
                            const ppf_verify_params* params, ppf_pose_score* scores, int* best, ppf_verify_stats* stats);

/* ---- surfel z-buffers of posed model clouds: self-occlusion-aware verification, depth and label images ---------- */
#define PPF_RENDER_MAX_SPLAT 8 /* a rendered row's candidate pixels reach at most this far from its centre pixel */

typedef struct ppf_render_params {
  float splat_radius; /* metres, finite, > 0: the surfel disk radius */
  float visible_tol;  /* metres, finite, > 0: a row is visible when z <= zbuf + visible_tol at its centre pixel */
  int32_t flags;      /* 0; reserved */
  int32_t reserved[4];
} ppf_render_params;

typedef struct ppf_render_stats {
  int32_t n_dets, n_jobs; /* detections given, poses rendered */
  int32_t n_launches;     /* kernel launches of the call */
  int32_t n_host_syncs;   /* blocking read-backs + synchronisations of the call (host-to-device uploads not counted) */
  float ms_wall;
  int32_t reserved[4];
} ppf_render_stats;

/* splat_radius 0.003, visible_tol 0.005, flags 0 */
void ppf_default_render_params(ppf_render_params* p);
/* ppf_verify_frame with self-occlusion: every row of dets[i].model_cloud moved by a pose is drawn as a
 * disk of splat_radius into a z-buffer of that pose alone (depth_rows x depth_cols, intr), and a scored row is
 * considered only when it is finite, faces the camera and is visible there (z <= zbuf + visible_tol at its centre pixel,
 * or that pixel is empty).  Everything else, the arguments, limits and outputs included, is ppf_verify_frame's, except:
 * the image size and intr are always required (depth may still be NULL: no depth test), fx and fy must be > 0, and
 * PPF_VERIFY_ALL_ROWS is PPF_ERR_INVALID.  Two blocking read-backs: the pose windows, then the scores. */
ppf_status ppf_verify_frame_rendered(const ppf_frame_detection* dets, int n_dets, const ppf_pose* poses, const int* n_poses, int top,
                                     const float* depth, int depth_rows, int depth_cols, const double* intr,
                                     const ppf_verify_params* params, const ppf_render_params* rparams, ppf_pose_score* scores,
                                     int* best, ppf_verify_stats* stats);
/* One z-buffer of rows x cols pixels (intr = {fx, fy, ppx, ppy}) for pose which[i] of every detection i with
 * which[i] >= 0 (poses is [n_dets][top] as ppf_match_frame returns it; best of either verify entry plugs in as which),
 * with the surfel coverage of ppf_verify_frame_rendered; equal depths go to the lowest detection index.  depth_out
 * (float32 metres, 0 where empty) and label_out (the detection index, -1 where empty) are packed HOST images and may
 * each be NULL.  Limits: n_dets 0..256, top 1..16, which[i] in [-1, top).  Argument errors are PPF_ERR_INVALID before
 * any device work; on any error the given images are all 0 and all -1.  stats may be NULL. */
ppf_status ppf_render_frame(const ppf_frame_detection* dets, int n_dets, const ppf_pose* poses, const int* which, int top, int rows,
                            int cols, const double* intr, const ppf_render_params* rparams, float* depth_out, int32_t* label_out,
                            ppf_render_stats* stats);

/* ---- one consistent set of poses per frame: duplicates, overlapping boxes and several instances per box ---------- */
#define PPF_SELECT_NONE 0       /* k >= n_poses[i]: the row is all zero */
#define PPF_SELECT_SELECTED 1
#define PPF_SELECT_GATED 2      /* key < min_score (or NaN), or n_supported < min_pixels */
#define PPF_SELECT_SUPPRESSED 3 /* conflicts with a hypothesis selected before it */

typedef struct ppf_select_params {
  float depth_tol;    /* metres, finite, > 0: a drawn pixel is supported when |depth - z| <= depth_tol */
  float max_overlap;  /* in [0, 1]: two hypotheses conflict above this share of the smaller supported set */
  float min_score;    /* finite; gate on the rank key */
  int32_t min_pixels; /* >= 1; gate on n_supported */
  int32_t flags;      /* 0; reserved */
  int32_t reserved[4];
} ppf_select_params;

typedef struct ppf_select_info {
  int32_t status, rank;        /* PPF_SELECT_*; rank: position in selection order, -1 unless selected */
  int32_t suppressed_by;       /* flat index i * top + k of the suppressor, else -1 */
  int32_t n_drawn, n_supported; /* pixels of the pose's own z-buffer; those the depth image agrees with */
  int32_t n_overlap;           /* supported pixels shared with the suppressor, else 0 */
  float explained, key;        /* n_supported / n_drawn; what the order ranks by */
  int32_t reserved[4];
} ppf_select_info;

typedef struct ppf_select_stats {
  int32_t n_dets, n_jobs;         /* detections given, hypotheses rendered */
  int32_t n_eligible, n_selected; /* hypotheses that passed the gate; those selected */
  int32_t n_launches;             /* kernel launches of the call */
  int32_t n_host_syncs;           /* blocking read-backs of the call (host-to-device uploads not counted) */
  float ms_wall;
  int32_t reserved[4];
} ppf_select_stats;

/* depth_tol 0.01, max_overlap 0.25, min_score 0, min_pixels 1, flags 0 */
void ppf_default_select_params(ppf_select_params* p);
/* Picks one consistent set among all hypotheses j = i * top + k, k < n_poses[i], of a frame.  Each is drawn
 * into a z-buffer of its own as ppf_verify_frame_rendered draws it; its supported pixels are the drawn ones whose depth
 * pixel is finite, > 0 and within depth_tol of the z-buffer.  explained = n_supported / n_drawn; the rank key is
 * scores[j].score when `scores` is given (what either verify entry returned), else explained.  Hypotheses that pass the
 * gate (key >= min_score, n_supported >= min_pixels) are taken greedily by key descending, then j ascending; one is
 * suppressed by the earliest selected hypothesis it shares more than max_overlap * min(n_supported) supported pixels with.
 * dets, poses, n_poses and top are what ppf_match_frame took and returned (only model_cloud is read).  depth: required
 * HOST image, float32 metres, packed depth_rows x depth_cols; intr = {fx, fy, ppx, ppy}, fx and fy > 0.
 * info is [n_dets][top]; selected is [n_dets * top], the selected flat indices in selection order, then -1;
 * depth_out (0 where empty) and label_out (the flat index j of the nearest selected hypothesis, -1 where empty) are
 * packed HOST images of the depth image's size and may each be NULL; stats may be NULL.  Limits: n_dets 0..256, top 1..16,
 * n_poses[i] 0..top.  Argument errors are PPF_ERR_INVALID before any device work; on any error every info row is zero,
 * selected is all -1, *n_selected is 0 and the given images are all 0 and all -1.  A hypothesis's counts do not depend
 * on the rest of the call, the launch count does not depend on n_dets, and there are two blocking read-backs: the pose
 * windows, then the results. */
ppf_status ppf_select_frame(const ppf_frame_detection* dets, int n_dets, const ppf_pose* poses, const int* n_poses, int top,
                            const ppf_pose_score* scores, const float* depth, int depth_rows, int depth_cols, const double* intr,
                            const ppf_render_params* rparams, const ppf_select_params* params, ppf_select_info* info, int* selected,
                            int* n_selected, float* depth_out, int32_t* label_out, ppf_select_stats* stats);

/* ---- projective point-to-plane refinement of the poses of a frame on the depth image itself ------------------------- */
#define PPF_REFINE_NONE 0       /* row with k >= n_poses[i] */
#define PPF_REFINE_CONVERGED 1  /* the last step was below eps_rot and eps_trans */
#define PPF_REFINE_MAX_ITERS 2
#define PPF_REFINE_LOST 3       /* too few pairs at an evaluation: the pose of that evaluation is returned */
#define PPF_REFINE_STEP 4       /* a step over the limits or not finite was refused: likewise */

typedef struct ppf_refine_params {
  float depth_gate;      /* metres, finite, > 0: a pair needs |d - z| <= depth_gate */
  float max_step_rot;    /* rad, finite, > 0 */
  float max_step_trans;  /* metres, finite, > 0 */
  float eps_rot, eps_trans; /* finite, >= 0 */
  float min_pair_share;  /* in [0, 1]: pairs needed as a share of the considered rows */
  int32_t min_pairs;     /* >= 6 */
  int32_t max_iters;     /* 0..100; 0 evaluates nothing and returns the poses as given, status MAX_ITERS */
  int32_t model_step;    /* >= 1, as ppf_verify_params */
  int32_t flags;         /* 0; reserved */
  int32_t reserved[4];
} ppf_refine_params;

typedef struct ppf_refine_info {
  int32_t status, iterations;        /* PPF_REFINE_*; steps applied */
  int32_t n_rows, n_considered;      /* model rows scored; finite rows facing the camera at the last evaluation */
  int32_t n_pairs_first, n_pairs_last;
  float rmse_first, rmse_last;       /* point-to-plane rms of the first / last evaluation, metres */
  int32_t reserved[4];
} ppf_refine_info;

typedef struct ppf_refine_stats {
  int32_t n_dets, n_jobs; /* detections given, poses refined */
  int32_t n_launches;     /* kernel launches of the call */
  int32_t n_host_syncs;   /* blocking read-backs of the call (host-to-device uploads not counted) */
  float ms_wall;
  int32_t reserved[4];
} ppf_refine_stats;

/* depth_gate 0.02, max_step_rot 0.35, max_step_trans 0.03, eps_rot 1e-5, eps_trans 1e-5, min_pair_share 0.25, min_pairs 16,
 * max_iters 20, model_step 1, flags 0 */
void ppf_default_refine_params(ppf_refine_params* p);
/* Refines pose k < n_poses[i] of detection i against the depth image alone (DESIGN.md §17 states every step bit for bit):
 * per iteration the rows 0, s, 2s, ... of dets[i].model_cloud are moved by the pose, a finite row that faces the camera is
 * paired with the depth pixel under it when that pixel is finite, > 0 and within depth_gate of the row's z, and one damped
 * point-to-plane step (the model's own moved normal; rotation about the moved centre of the model) is solved and applied,
 * until a step is below eps_rot and eps_trans (CONVERGED) or max_iters steps were applied (MAX_ITERS).  An evaluation with
 * fewer than min_pairs pairs or fewer than min_pair_share of the considered rows ends the pose LOST; a step that is not
 * finite or exceeds max_step_rot / max_step_trans ends it STEP; either way the pose of that evaluation is returned.
 * dets, poses, n_poses and top are what ppf_verify_frame takes (only model_cloud is read).  depth: required HOST image,
 * float32 metres, packed depth_rows x depth_cols; intr = {fx, fy, ppx, ppy}, fx and fy finite and non-zero.
 * out is [n_dets][top] and may be `poses` itself: a pose with iterations > 0 gets the refined matrix and q, t and angle
 * from it; alpha, model_index and num_votes are copied; residual is rmse_last; with iterations == 0 the rest of the record
 * is the one given (max_iters == 0 leaves the residual too); rows with k >= n_poses[i] are copied.  info ([n_dets][top]) and
 * stats may be NULL.  Limits: n_dets 0..256, top 1..16, n_poses[i] 0..top.  Argument errors are PPF_ERR_INVALID before any
 * device work; on any error out is a copy of poses and every info row is zero.  A pose's result depends neither on the
 * other poses of the call nor on scheduling; one launch and one read-back whatever n_dets is. */
ppf_status ppf_refine_frame(const ppf_frame_detection* dets, int n_dets, const ppf_pose* poses, const int* n_poses, int top,
                            const float* depth, int depth_rows, int depth_cols, const double* intr,
                            const ppf_refine_params* params, ppf_pose* out, ppf_refine_info* info, ppf_refine_stats* stats);

/* ---- a raw sensor depth image aligned to the colour camera (what the vendor SDK's depth_image_to_color_camera does) -- */
#define PPF_CAMERA_NEWTON_ITERS 7   /* Newton steps of an unprojection, always all of them (DESIGN.md §18 measures the count) */
#define PPF_REGISTER_MAX_QUAD_PX 16 /* a triangle whose clamped bounding box is wider or taller than this is not drawn */

/* A pinhole camera with OpenCV's rational radial + tangential distortion (include/ppf_camera_math.h is the arithmetic,
 * fp64, bit for bit the same on the host and on the device).  A camera is valid when fx and fy are finite and non-zero,
 * every other field is finite, max_r >= 0 and reserved is zero. */
typedef struct ppf_camera {
  double fx, fy, cx, cy;                 /* fx, fy finite and non-zero; cx, cy finite */
  double k1, k2, p1, p2, k3, k4, k5, k6; /* OpenCV order: rational radial + tangential; all zero: pinhole */
  double max_r;                          /* 0: no limit; else a normalised point with x*x + y*y > max_r*max_r is invalid */
  double reserved[3];                    /* 0 */
} ppf_camera;
/* a pinhole camera: every coefficient, max_r and reserved zero */
void ppf_default_camera(ppf_camera* cam, double fx, double fy, double cx, double cy);
/* Host only, no device needed.  xy and uv are [n][2] doubles; valid ([n] bytes, 1 or 0) may be NULL.
 * ppf_camera_project: normalised points (x, y) -> pixels (u, v); ppf_camera_unproject: pixels -> normalised points by
 * exactly PPF_CAMERA_NEWTON_ITERS Newton steps.  An invalid point (ppf_camera_math.h lists the conditions) gives NaN NaN
 * and valid 0.  A NULL pointer, n < 0 or an invalid camera is PPF_ERR_INVALID, the outputs all NaN and 0 where they can be
 * reached. */
ppf_status ppf_camera_project(const ppf_camera* cam, const double* xy, int n, double* uv, uint8_t* valid);
ppf_status ppf_camera_unproject(const ppf_camera* cam, const double* uv, int n, double* xy, uint8_t* valid);
/* Carries n boxes {x, y, width, height} of the image of camera `from` (e.g. a detector's boxes on the raw, distorted colour
 * image) into the to_rows x to_cols image of camera `to`: the eight points of a box (corners and side midpoints, at x,
 * x + w / 2.0, x + w and likewise for y) are unprojected with `from` and projected with `to`; the result spans
 * floor(min) .. ceil(max) of the valid ones, clamped to the image (as doubles, before the conversion to int).  Rounding is
 * outwards: a point that comes back one ulp past an integer grows the box by a pixel.  A box without a valid point, or
 * empty after clamping, is {0, 0, 0, 0}.  Host only.  Argument errors are PPF_ERR_INVALID and every output box is zero. */
ppf_status ppf_camera_map_boxes(const ppf_camera* from, const ppf_camera* to, int to_rows, int to_cols, const int* boxes_xywh, int n,
                                int* out_xywh);

typedef struct ppf_depth_map ppf_depth_map; /* opaque, device-resident: the ray table of a depth camera + the calibration */

/* Built once per calibration.  R9 (row-major) and t3 (metres) take a point of the depth camera's frame into the colour
 * camera's: Q[r] = R[r][0]*P0 + R[r][1]*P1 + R[r][2]*P2 + t[r].  R9 is used as given: it is NOT tested for orthonormality.
 * One kernel (k_reg_rays) unprojects every depth pixel once; the table takes 16 bytes a pixel.  Argument errors (NULL
 * pointers, sizes <= 0 or above INT32_MAX pixels, an invalid camera, R9 or t3 not finite) are PPF_ERR_INVALID before any
 * device work; on any error *out is NULL.  A map is immutable: any number of host threads may register with it at once. */
ppf_status ppf_depth_map_create(const ppf_camera* depth_cam, int depth_rows, int depth_cols, const ppf_camera* color_cam,
                                int color_rows, int color_cols, const double* R9, const double* t3, ppf_depth_map** out);
ppf_status ppf_depth_map_release(ppf_depth_map* map);
/* the ray table, HOST [depth_rows][depth_cols][2] doubles: the normalised (x, y) of every depth pixel, NaN NaN = invalid */
ppf_status ppf_depth_map_rays(const ppf_depth_map* map, double* rays);

typedef struct ppf_register_params {
  float quad_dz_abs, quad_dz_rel; /* finite, >= 0: a quad is cut when max(zc) - min(zc) > quad_dz_abs + quad_dz_rel * min(zc) */
  int32_t flags;                  /* 0 */
  int32_t reserved[4];
} ppf_register_params;

typedef struct ppf_register_stats {
  int32_t n_vertices;       /* depth pixels that are kept, have a valid ray and project validly into the colour camera */
  int32_t n_quads;          /* quads of four valid vertices */
  int32_t n_quads_cut;      /* of those, cut at a depth discontinuity */
  int32_t n_quads_oversize; /* of the uncut ones, with a triangle over PPF_REGISTER_MAX_QUAD_PX */
  int32_t n_filled;         /* output pixels drawn */
  int32_t n_launches;       /* kernel launches of the call */
  int32_t n_host_syncs;     /* blocking waits of the call */
  float ms_wall;
  int32_t reserved[4];
} ppf_register_stats;

/* 0.02, 0.02, 0: a choice, not tuned on real data (2 cm plus 2 % of the depth between the vertices of one quad) */
void ppf_default_register_params(ppf_register_params* p);
/* Draws the depth image of the map's depth camera into the pixel grid of its colour camera (DESIGN.md §18 states every
 * step bit for bit): every kept pixel becomes a vertex in the colour frame, every quad of four valid vertices that is not
 * cut is drawn as two triangles with linear depth interpolation, and each output pixel takes the nearest depth drawn on it.
 * out: float32 metres, packed color_rows x color_cols, 0 where nothing was drawn: exactly what ppf_cloud_from_depth and
 * every frame stage take, with intr = the first four doubles of color_cam.  depth, row_pitch_bytes and dp are
 * ppf_cloud_from_depth's (format, depth_scale, z_min, z_max; the image is depth_rows x depth_cols of the map), except
 * that dp->flags must be 0.  The result does not depend on scheduling.  Three launches, one blocking wait and one
 * read-back whatever the sizes.  Argument errors are PPF_ERR_INVALID before any device work; on any error `out` is all 0
 * where it can be reached and *stats is zero.  stats may be NULL. */
ppf_status ppf_depth_register(const ppf_depth_map* map, const void* depth, size_t row_pitch_bytes, const ppf_depth_params* dp,
                              const ppf_register_params* rp, float* out, ppf_register_stats* stats);
/* the same between DEVICE buffers: enqueued on `stream` (a hipStream_t, NULL: default stream), returns when the image is
 * complete.  d_out (color_rows x color_cols floats, packed) serves as the z-buffer while the call runs.  A pointer the
 * current device cannot read, a buffer that runs past the end of its allocation, or d_out overlapping the depth image is
 * PPF_ERR_INVALID before anything is launched; d_out is not touched on an error. */
ppf_status ppf_depth_register_device(const ppf_depth_map* map, const void* d_depth, size_t row_pitch_bytes, const ppf_depth_params* dp,
                                     const ppf_register_params* rp, float* d_out, void* stream, ppf_register_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* PPF_HIP_H */
